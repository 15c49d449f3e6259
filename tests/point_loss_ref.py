"""Case table, references and checks of the voxel-wise loss kernels (csrc/kernels/loss_point.h, launchers in csrc/icl_abi.inc), of
``ops.softmax_kl`` / ``ops.entropy`` / ``ops.focal_loss`` and of the functions of ``icl_amd.utils.losses`` built on them, shared by
test_point_loss_emu.py (CPU emulation of the kernel sources) and test_gpu_point_loss.py (the MI355X): both run every entry of ``CHECKS``;
``GPU_CHECKS`` holds the two shapes at which the grid-stride loops wrap around, too slow for the emulation.

References: the formulas of the losses restated in torch fp64 with autograd (``ref_kl``, ``ref_entropy``, ``ref_focal``).  The focal
restatement builds (1 - pt) from a DETACHED pt, as the reference module takes it from ``.data``: a kernel that differentiates the
modulating factor misses the gradient bound by a wide margin.  tests/golden/point_losses.npz holds what the reference's own functions
gave on the small inputs (make_golden_point_losses.py); ``check_golden`` ties the restatements to it.

Bounds at the small shapes, the project's own for this kernel family (test_fused_losses):
    |value - ref| < 1e-5 * max(1, |ref|)      a loss of order 1; a sum-reduced focal loss or the 66.67 of the extreme logits relative to
                                              its magnitude (one fp32 ulp of 66.67 is 7.6e-6)
    max|grad - ref| / max|ref| < 1e-4         (max|ref| no smaller than the smallest normal fp32 number)
Every case runs forward and backward with an upstream gradient of 1.3 (maps: a non-uniform one), and twice: the two runs agree bit for bit.
At the two large shapes of GPU_CHECKS the bound is 2 N, N = the error of a plain torch fp32 evaluation of the same formula against the
fp64 restatement at that shape (LARGE_N below)."""
import contextlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from icl_amd import _lib, ops  # noqa: E402
from icl_amd.utils import losses as L  # noqa: E402
from icl_amd.utils.hashfill import synthetic_labels, synthetic_volume  # noqa: E402

B, S = 2, (6, 5, 7)        # 210 voxels per sample: no multiple of 64, and a sample boundary inside a block
G = 1.3                    # upstream gradient of every scalar
VALUE_TOL, GRAD_TOL = 1e-5, 1e-4
F32_TINY = float(np.finfo(np.float32).tiny)     # a gradient whose largest reference entry is below the smallest normal fp32 number (the target's
#                                                 gradient at the extreme logits alone: 3e-42) is compared on that scale, not on its own
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "point_losses.npz")


# ---- references (fp64 when fed fp64, the plain torch fp32 evaluation when fed fp32) --------------------------------------------------------

def ref_kl(a, b, w_fwd=1.0, w_rev=0.0, dim=1):
    """w_fwd mean KL(q||p) + w_rev mean KL(p||q), p = softmax(a), q = softmax(b); the means over all elements."""
    la, lb = torch.log_softmax(a, dim), torch.log_softmax(b, dim)
    return w_fwd * (lb.exp() * (lb - la)).mean() + w_rev * (la.exp() * (la - lb)).mean()


def ref_entropy_map(x, from_logits=False, scale=1.0):
    p = torch.softmax(x, 1) if from_logits else x
    return -scale * (p * torch.log(p + 1e-6)).sum(1, keepdim=True)


def ref_entropy(x, from_logits=False, scale=1.0):
    return ref_entropy_map(x, from_logits, scale).mean()


def ref_focal(logits, labels, gamma, alpha=None, size_average=True):
    """-alpha_y (1 - pt)^gamma log pt with pt DETACHED; labels outside [0, nc) add 0 and still count in the mean.  ``alpha``: a list of
    Python floats, rounded to fp32 first as the reference module holds it."""
    nc = logits.shape[1]
    lp = torch.log_softmax(logits, 1).movedim(1, -1).reshape(-1, nc)
    y = labels.reshape(-1)
    ok = (y >= 0) & (y < nc)
    ys = torch.where(ok, y, torch.zeros_like(y))
    logpt = lp.gather(1, ys[:, None])[:, 0]
    pt = logpt.detach().exp()
    w = torch.ones_like(logpt)
    if alpha is not None:
        w = torch.tensor(alpha, dtype=torch.float32, device=logits.device).to(logits.dtype)[ys]
    loss = torch.where(ok, -w * (1 - pt) ** gamma * logpt, torch.zeros_like(logpt))
    return loss.mean() if size_average else loss.sum()


def ref_compute_kl(ps, qs):
    return sum(ref_kl(a, b, 0.5, 0.5, dim=-1) for a, b in zip(ps, qs)) / len(ps)


# ---- running a function and its backward ---------------------------------------------------------------------------------------------------

def logits(shape, seed, scale=2.0):
    return synthetic_volume(tuple(shape), seed) * scale


def probs(shape, seed):
    """Probabilities over dim 1 with one exact 0 (and the voxel renormalised by hand, so that it stays a distribution)."""
    p = torch.softmax(logits(shape, seed), 1).contiguous()
    first = (0, slice(None)) + (0,) * (p.dim() - 2)
    v = p[first].clone()
    v[1] += v[0]
    v[0] = 0.0
    p[first] = v
    return p


def evaluate(fn, tensors, needs, dev, dtype=torch.float32, upstream=G):
    """out = fn(*tensors on dev); (out * upstream).sum().backward().  ``fn`` may return a tuple of outputs, ``upstream`` then is a tuple.
    Returns (outputs, gradients) on the CPU: the gradient of an input that needs none — or got none — is None."""
    xs = []
    for t, need in zip(tensors, needs):
        t = t.to(device=dev, dtype=dtype) if t.is_floating_point() else t.to(dev)
        xs.append(t.clone().requires_grad_() if need else t)
    out = fn(*xs)
    outs = out if isinstance(out, tuple) else (out,)
    ups = upstream if isinstance(upstream, tuple) else (upstream,)
    obj = 0
    for o, u in zip(outs, ups):
        u = u.to(device=o.device, dtype=o.dtype) if torch.is_tensor(u) else u
        obj = obj + (o * u).sum()
    obj.backward()
    return [o.detach().cpu() for o in outs], [x.grad.detach().cpu() if (need and x.grad is not None) else None for x, need in zip(xs, needs)]


def errors(got, want):
    """(value errors relative to max(1, |ref|), gradient errors max|d| / max|ref|) of two results of ``evaluate``."""
    ve, ge = [], []
    for g, w in zip(got[0], want[0]):
        w = w.double()
        ve.append(float((g.double() - w).abs().max() / max(1.0, float(w.abs().max()))))
    for g, w in zip(got[1], want[1]):
        assert (g is None) == (w is None), "a gradient is missing or unexpected"
        if w is not None:
            w = w.double()
            ge.append(float((g.double() - w).abs().max() / max(float(w.abs().max()), F32_TINY)))
    return ve, ge


def bit_equal(x, y):
    assert len(x[0]) == len(y[0]) and len(x[1]) == len(y[1])
    for a, b in zip(x[0] + x[1], y[0] + y[1]):
        assert (a is None) == (b is None)
        if a is not None:
            assert torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)), "two evaluations differ in bits"


def check(case, fn, ref, tensors, needs, dev, upstream=G):
    """Kernel result against the fp64 restatement within the bounds, finite, and bit-reproducible.  Returns the kernel result."""
    got = evaluate(fn, tensors, needs, dev, upstream=upstream)
    bit_equal(got, evaluate(fn, tensors, needs, dev, upstream=upstream))
    want = evaluate(ref, tensors, needs, "cpu", dtype=torch.float64, upstream=upstream)
    for t in got[0] + [g for g in got[1] if g is not None]:
        assert bool(torch.isfinite(t).all()), case
    ve, ge = errors(got, want)
    print(f"{case}: value err {['%.2e' % v for v in ve]} (asserted < {VALUE_TOL:g}), grad err {['%.2e' % g for g in ge]} (asserted < {GRAD_TOL:g})")
    assert all(v < VALUE_TOL for v in ve) and all(g < GRAD_TOL for g in ge), (case, ve, ge)
    return got


@contextlib.contextmanager
def forced_generic():
    """ICL_LOSS_GENERIC=1: the class-walking body for any class count (read per call by the launchers)."""
    old = os.environ.get("ICL_LOSS_GENERIC")
    os.environ["ICL_LOSS_GENERIC"] = "1"
    try:
        yield
    finally:
        if old is None:
            del os.environ["ICL_LOSS_GENERIC"]
        else:
            os.environ["ICL_LOSS_GENERIC"] = old


def register_and_generic(case, fn, ref, tensors, needs, dev, upstream=G):
    """nc = 3 through the register body and, under ICL_LOSS_GENERIC=1, through the class-walking body: each within the bounds of the
    reference, and of each other (not bit for bit: the online normaliser sums in another order)."""
    assert os.environ.get("ICL_LOSS_GENERIC") != "1"
    reg = check(case + " registers", fn, ref, tensors, needs, dev, upstream)
    with forced_generic():
        gen = check(case + " class walk", fn, ref, tensors, needs, dev, upstream)
    ve, ge = errors(gen, reg)
    print(f"{case}: class walk against registers: value {ve}, grad {ge}")
    assert all(v < VALUE_TOL for v in ve) and all(g < GRAD_TOL for g in ge), (case, ve, ge)


# ---- KL --------------------------------------------------------------------------------------------------------------------------------------

def kl_inputs(nc):
    return [logits((B, nc) + S, 100 + nc), logits((B, nc) + S, 200 + nc)]


def check_kl(nc, dev):
    """softmax_kl_loss: target with a gradient (the reference does not detach it) and without — then no second gradient exists, and the
    first has the same bits."""
    t = kl_inputs(nc)
    both = check(f"kl nc={nc}, target requires grad", L.softmax_kl_loss, ref_kl, t, (True, True), dev)
    one = check(f"kl nc={nc}, target without grad", L.softmax_kl_loss, ref_kl, t, (True, False), dev)
    assert both[1][1] is not None and one[1][1] is None
    bit_equal(([both[0][0]], [both[1][0]]), ([one[0][0]], [one[1][0]]))
    check(f"kl nc={nc}, gradient to the target only", L.softmax_kl_loss, ref_kl, t, (False, True), dev)


def check_kl_generic(dev):
    register_and_generic("kl nc=3", L.softmax_kl_loss, ref_kl, kl_inputs(3), (True, True), dev)
    register_and_generic("kl nc=3 symmetric, last axis", lambda a, b: ops.softmax_kl(a, b, 0.5, 0.5, dim=-1),
                         lambda a, b: ref_kl(a, b, 0.5, 0.5, dim=-1), [logits((37, 3), 31), logits((37, 3), 32)], (True, True), dev)


def check_kl_extreme(dev):
    """Logits [100, -100, 0] against [-100, 100, 0]: 66.6667 in the reference (a class whose probability underflows adds 0 * finite = 0),
    alone and beside a voxel of equal logits and ordinary ones; both directions."""
    a = torch.tensor([100.0, -100.0, 0.0]).reshape(1, 3, 1)
    b = torch.tensor([-100.0, 100.0, 0.0]).reshape(1, 3, 1)
    got = check("kl extreme logits", L.softmax_kl_loss, ref_kl, [a, b], (True, True), dev)
    assert abs(float(got[0][0]) - 200.0 / 3.0) < 1e-4, got[0]
    a4 = torch.cat([a, torch.full((1, 3, 1), 0.7), logits((1, 3, 5), 41)], 2).contiguous()
    b4 = torch.cat([b, torch.full((1, 3, 1), -1.9), logits((1, 3, 5), 42)], 2).contiguous()
    check("kl extreme + equal + ordinary logits", L.softmax_kl_loss, ref_kl, [a4, b4], (True, True), dev)
    check("kl extreme, symmetric", lambda x, y: ops.softmax_kl(x, y, 0.5, 0.5), lambda x, y: ref_kl(x, y, 0.5, 0.5), [a4, b4], (True, True), dev)


def compute_kl_inputs():
    shapes = ((37, 5), (4, 9, 6), (37, 5))
    return [logits(s, 300 + i) for i, s in enumerate(shapes)] + [logits(s, 310 + i) for i, s in enumerate(shapes)]


def check_compute_kl(dev):
    """compute_kl_loss on lists of three tensors, [37, 5] and [4, 9, 6], soft-max over the last axis (inner = 1): gradients reach both
    arguments; and a list of one."""
    t = compute_kl_inputs()
    got = check("compute_kl_loss, three pairs", lambda *x: L.compute_kl_loss(list(x[:3]), list(x[3:])),
                lambda *x: ref_compute_kl(x[:3], x[3:]), t, (True,) * 6, dev)
    assert all(g is not None and float(g.abs().max()) > 0 for g in got[1])
    check("compute_kl_loss, one pair", lambda x, y: L.compute_kl_loss([x], [y]), lambda x, y: ref_compute_kl([x], [y]), [t[1], t[4]],
          (True, True), dev)


# ---- entropy ---------------------------------------------------------------------------------------------------------------------------------

def map_upstream(seed=77):
    """The non-uniform upstream gradient of a [B, 1, S] map."""
    return 0.5 + synthetic_volume((B, 1) + S, seed).abs()


def check_entropy(nc, dev):
    """Probabilities (with an exact 0) through the four functions of losses.py, C = 2 and C = nc; logits through ops.entropy(from_logits);
    mean, map (non-uniform upstream), and both from one pass."""
    p, x, up = probs((B, nc) + S, 400 + nc), logits((B, nc) + S, 500 + nc), map_upstream()
    assert float(p.min()) == 0.0
    check(f"entropy_minmization nc={nc}", L.entropy_minmization, ref_entropy, [p], (True,), dev)
    got = check(f"entropy_map nc={nc}", L.entropy_map, ref_entropy_map, [p], (True,), dev, upstream=up)
    assert tuple(got[0][0].shape) == (B, 1) + S
    for C in sorted({2, nc}):
        sc = 1.0 / np.log(C)
        check(f"entropy_loss nc={nc} C={C}", lambda t: L.entropy_loss(t, C=C), lambda t: ref_entropy(t, False, sc), [p], (True,), dev)
        check(f"entropy_loss_map nc={nc} C={C}", lambda t: L.entropy_loss_map(t, C=C), lambda t: ref_entropy_map(t, False, sc), [p], (True,),
              dev, upstream=up)
    check(f"entropy from logits, mean, nc={nc}", lambda t: ops.entropy(t, from_logits=True), lambda t: ref_entropy(t, True), [x], (True,), dev)
    check(f"entropy from logits, map, nc={nc}", lambda t: ops.entropy(t, from_logits=True, scale=0.7, want="map"),
          lambda t: ref_entropy_map(t, True, 0.7), [x], (True,), dev, upstream=up)
    for fl, t in ((False, p), (True, x)):
        check(f"entropy mean and map in one pass, from_logits={fl}, nc={nc}", lambda v: ops.entropy(v, from_logits=fl, want="both"),
              lambda v: (ref_entropy(v, fl), ref_entropy_map(v, fl)), [t], (True,), dev, upstream=(G, up))


def check_entropy_generic(dev):
    p, x, up = probs((B, 3) + S, 403), logits((B, 3) + S, 503), map_upstream()
    register_and_generic("entropy nc=3 probabilities", lambda v: ops.entropy(v, want="both"),
                         lambda v: (ref_entropy(v), ref_entropy_map(v)), [p], (True,), dev, upstream=(G, up))
    register_and_generic("entropy nc=3 logits", lambda v: ops.entropy(v, from_logits=True, want="both"),
                         lambda v: (ref_entropy(v, True), ref_entropy_map(v, True)), [x], (True,), dev, upstream=(G, up))


# ---- focal -----------------------------------------------------------------------------------------------------------------------------------

FOCAL_ALPHA = {2: 0.25, 3: [0.2, 0.5, 0.3]}      # a float at nc = 2 ([alpha, 1 - alpha]), a list at nc = 3


def focal_alpha_list(alpha):
    return [alpha, 1 - alpha] if isinstance(alpha, (float, int)) else alpha


def focal_inputs(nc, seed=0):
    return [logits((B, nc) + S, 600 + nc + seed), synthetic_labels((B,) + S, 700 + nc + seed, nc)]


def check_focal(nc, dev):
    """gamma 0, 2, 1.5; alpha none and (nc = 2: a float, nc = 3: a list); mean and sum."""
    t = focal_inputs(nc)
    for gamma in (0, 2, 1.5):
        for alpha in (None,) + ((FOCAL_ALPHA[nc],) if nc in FOCAL_ALPHA else ()):
            for avg in (True, False):
                al = None if alpha is None else focal_alpha_list(alpha)
                check(f"focal nc={nc} gamma={gamma} alpha={alpha} mean={avg}", lambda a, y: L.FocalLoss(gamma, alpha, avg)(a, y),
                      lambda a, y: ref_focal(a, y, gamma, al, avg), t, (True, False), dev)


def check_focal_generic(dev):
    for gamma, avg in ((2, True), (1.5, False)):
        register_and_generic(f"focal nc=3 gamma={gamma}", lambda a, y: L.FocalLoss(gamma, FOCAL_ALPHA[3], avg)(a, y),
                             lambda a, y: ref_focal(a, y, gamma, FOCAL_ALPHA[3], avg), focal_inputs(3), (True, False), dev)


def check_focal_rows(dev):
    """[M, C] input: the class axis is the last one (inner = 1)."""
    a, y = logits((37, 5), 801), synthetic_labels((37,), 802, 5)
    check("focal [37, 5]", lambda v, t: L.FocalLoss(2, [0.1, 0.2, 0.3, 0.25, 0.15])(v, t),
          lambda v, t: ref_focal(v, t, 2, [0.1, 0.2, 0.3, 0.25, 0.15]), [a, y], (True, False), dev)
    check("focal [37, 5] gamma=1.5 sum", lambda v, t: L.FocalLoss(1.5, None, False)(v, t), lambda v, t: ref_focal(v, t, 1.5, None, False),
          [a, y], (True, False), dev)


def check_focal_edges(dev):
    """A label map of a single class; a voxel whose logit makes pt round to 1 (factor 0 for gamma > 0, 1 for gamma = 0); two labels
    outside [0, nc): value and gradient equal the reference with those voxels masked, and the gradient there is exactly 0."""
    a, y = focal_inputs(3, seed=50)
    one = torch.full_like(y, 2)
    check("focal single-class labels", lambda v, t: L.FocalLoss(2, FOCAL_ALPHA[3])(v, t), lambda v, t: ref_focal(v, t, 2, FOCAL_ALPHA[3]),
          [a, one], (True, False), dev)
    a1 = a.clone()
    a1[0, :, 1, 2, 3] = torch.tensor([-30.0, 60.0, -30.0])
    y1 = y.clone()
    y1[0, 1, 2, 3] = 1
    assert float(torch.softmax(a1[0, :, 1, 2, 3], 0)[1]) == 1.0
    for gamma in (0, 2, 1.5):
        check(f"focal pt == 1, gamma={gamma}", lambda v, t: L.FocalLoss(gamma)(v, t), lambda v, t: ref_focal(v, t, gamma), [a1, y1],
              (True, False), dev)
    y2 = y.clone()
    y2[0, 0, 0, 1], y2[1, 5, 4, 6] = -1, 3
    for avg in (True, False):
        got = check(f"focal labels outside [0, nc), mean={avg}", lambda v, t: L.FocalLoss(1.5, FOCAL_ALPHA[3], avg)(v, t),
                    lambda v, t: ref_focal(v, t, 1.5, FOCAL_ALPHA[3], avg), [a, y2], (True, False), dev)
        g = got[1][0]
        assert float(g[0, :, 0, 0, 1].abs().max()) == 0.0 and float(g[1, :, 5, 4, 6].abs().max()) == 0.0
        assert float(g.abs().max()) > 0.0


# ---- non-contiguous inputs, refusals ----------------------------------------------------------------------------------------------------------

def check_noncontiguous(dev):
    """A permuted view gives the bits of its contiguous copy, for each mode."""
    nc = 3
    up = map_upstream()

    def view_of(x):      # inside the function under test: evaluate() clones its inputs, and a clone would be contiguous
        v = x.permute(0, 2, 3, 4, 1).contiguous().permute(0, 4, 1, 2, 3)
        assert not v.is_contiguous()
        return v

    ab, p = kl_inputs(nc), [probs((B, nc) + S, 403)]
    y = synthetic_labels((B,) + S, 703, nc).permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1).to(dev)
    assert not y.is_contiguous()
    bit_equal(evaluate(lambda x, z: L.softmax_kl_loss(view_of(x), view_of(z)), ab, (True, True), dev),
              evaluate(L.softmax_kl_loss, ab, (True, True), dev))
    bit_equal(evaluate(lambda x: ops.entropy(view_of(x), want="both"), p, (True,), dev, upstream=(G, up)),
              evaluate(lambda x: ops.entropy(x, want="both"), p, (True,), dev, upstream=(G, up)))
    bit_equal(evaluate(lambda x: L.FocalLoss(2, FOCAL_ALPHA[3])(view_of(x), y), ab[:1], (True,), dev),
              evaluate(lambda x: L.FocalLoss(2, FOCAL_ALPHA[3])(x, y.contiguous()), ab[:1], (True,), dev))


def check_refusals(dev):
    """257 classes, sigmoid=True, a wrong ``consistency``: refused with an error, by the wrappers and by the entry points themselves."""
    import pytest
    from icl_amd.trainer import ICLConfig, ICLTrainer
    a = torch.zeros((1, 257, 4), device=dev)
    y = torch.zeros((1, 4), dtype=torch.int64, device=dev)
    for fn in (lambda: L.softmax_kl_loss(a, a), lambda: L.compute_kl_loss([a.reshape(4, 257)], [a.reshape(4, 257)]),
               lambda: L.entropy_minmization(a), lambda: L.entropy_map(a), lambda: ops.entropy(a, from_logits=True),
               lambda: L.FocalLoss()(a, y)):
        with pytest.raises(ValueError, match="257 classes"):
            fn()
    lib = _lib.lib()
    f = torch.zeros(1100, device=dev)
    ptr = ops._ptr
    assert lib.icl_kl_fwd(ptr(f), ptr(f), ptr(f), ptr(f), 1, 257, 4, 1.0, 0.0, None) == -1 and b"257 classes" in lib.icl_last_error()
    assert lib.icl_kl_bwd(ptr(f), ptr(f), ptr(f), ptr(f), None, 1, 0, 4, 1.0, 0.0, None) == -1
    assert lib.icl_kl_bwd(ptr(f), ptr(f), ptr(f), None, None, 1, 2, 4, 1.0, 0.0, None) == -1 and b"kl_bwd" in lib.icl_last_error()
    assert lib.icl_entropy_fwd(ptr(f), ptr(f), ptr(f), None, 1, 257, 4, 0, 1.0, None) == -1
    assert lib.icl_entropy_fwd(ptr(f), ptr(f), None, None, 1, 2, 4, 0, 1.0, None) == -1 and b"entropy_fwd" in lib.icl_last_error()
    assert lib.icl_entropy_bwd(ptr(f), None, None, ptr(f), 1, 2, 4, 0, 1.0, None) == -1
    assert lib.icl_focal_fwd(ptr(f), None, None, ptr(f), ptr(f), 1, 2, 4, 2.0, 1, None) == -1 and b"focal_fwd" in lib.icl_last_error()
    assert lib.icl_focal_bwd(ptr(f), ptr(y), None, ptr(f), ptr(f), 1, 257, 4, 2.0, 1, None) == -1
    assert lib.icl_kl_fwd(ptr(f), None, ptr(f), ptr(f), 1, 2, 4, 1.0, 0.0, None) == -1
    b2 = torch.zeros((1, 2, 4), device=dev)
    with pytest.raises(NotImplementedError):
        L.softmax_kl_loss(b2, b2, sigmoid=True)
    with pytest.raises(ValueError, match="alpha"):
        L.FocalLoss(2, [0.5])(b2, y)
    with pytest.raises(ValueError, match="consistency"):
        ICLTrainer(torch.nn.Linear(2, 2), ICLConfig(consistency="cosine"))


def check_dice_loss(dev):
    """dice_loss, the squared-denominator twin of dice_loss1 (a torch expression)."""
    p, t = probs((B, 2) + S, 402)[:, 1], synthetic_labels((B,) + S, 702, 2)
    def ref(s, y):
        y = y.to(s.dtype)
        return 1 - (2 * (s * y).sum() + 1e-5) / ((s * s).sum() + (y * y).sum() + 1e-5)
    got = evaluate(L.dice_loss, [p, t], (True, False), "cpu")
    want = evaluate(ref, [p, t], (True, False), "cpu", dtype=torch.float64)
    ve, ge = errors(got, want)
    assert ve[0] < VALUE_TOL and ge[0] < GRAD_TOL, (ve, ge)


# ---- the golden of the reference's own functions ------------------------------------------------------------------------------------------------

def golden_cases():
    """name -> (restatement, inputs, needs, upstream): what make_golden_point_losses.py feeds to the reference's functions, in fp64 on the
    CPU, and what ``check_golden`` feeds to the restatements."""
    cases = {}
    for nc in (2, 3, 16):
        cases[f"kl{nc}"] = (ref_kl, kl_inputs(nc), (True, True), G)
    a = torch.tensor([100.0, -100.0, 0.0]).reshape(1, 3, 1)
    cases["kl_extreme"] = (ref_kl, [a, -a], (True, True), G)
    cases["compute_kl"] = (lambda *x: ref_compute_kl(x[:3], x[3:]), compute_kl_inputs(), (True,) * 6, G)
    cases["entropy_min3"] = (ref_entropy, [probs((B, 3) + S, 403)], (True,), G)
    cases["entropy_map3"] = (ref_entropy_map, [probs((B, 3) + S, 403)], (True,), map_upstream())
    for nc, gamma, avg in ((2, 2, True), (3, 1.5, False), (3, 0, True)):
        al = focal_alpha_list(FOCAL_ALPHA[nc])
        cases[f"focal{nc}_g{gamma}_{'mean' if avg else 'sum'}"] = (
            (lambda v, t, gamma=gamma, al=al, avg=avg: ref_focal(v, t, gamma, al, avg)), focal_inputs(nc), (True, False), G)
    cases["focal_rows"] = (lambda v, t: ref_focal(v, t, 2, None, True), [logits((37, 5), 801), synthetic_labels((37,), 802, 5)], (True, False), G)
    return cases


def check_golden():
    """The fp64 restatements reproduce what the reference's own softmax_kl_loss, compute_kl_loss, FocalLoss, entropy_minmization and
    entropy_map gave in fp64 on the same inputs: 1e-12 relative (both are fp64 evaluations of one formula; the measured differences are
    below 1e-15).  entropy_loss / entropy_loss_map call .cuda() in the reference; they are the other two divided by log C, which
    ``ref_entropy(.., scale)`` restates and check_entropy pins through that factor."""
    gold = np.load(GOLDEN)
    for name, (ref, tensors, needs, up) in golden_cases().items():
        for i, t in enumerate(tensors):
            assert np.array_equal(gold[f"{name}.in{i}"], t.numpy()), (name, i)
        outs, grads = evaluate(ref, tensors, needs, "cpu", dtype=torch.float64, upstream=up)
        e = float(np.abs(outs[0].numpy() - gold[f"{name}.out"]).max() / max(1e-300, np.abs(gold[f"{name}.out"]).max()))
        worst = [e]
        for i, g in enumerate(grads):
            if g is not None:
                w = gold[f"{name}.grad{i}"]
                worst.append(float(np.abs(g.numpy() - w).max() / np.abs(w).max()))
        print(f"golden {name}: value {worst[0]:.2e}, gradients {['%.2e' % x for x in worst[1:]]} (asserted < 1e-12)")
        assert max(worst) < 1e-12, (name, worst)


CHECKS = {
    **{f"kl_nc{nc}": (lambda dev, nc=nc: check_kl(nc, dev)) for nc in (2, 3, 16, 17)},
    "kl_generic_nc3": check_kl_generic,
    "kl_extreme": check_kl_extreme,
    "compute_kl": check_compute_kl,
    **{f"entropy_nc{nc}": (lambda dev, nc=nc: check_entropy(nc, dev)) for nc in (2, 3, 16, 17)},
    "entropy_generic_nc3": check_entropy_generic,
    **{f"focal_nc{nc}": (lambda dev, nc=nc: check_focal(nc, dev)) for nc in (2, 3, 16, 17)},
    "focal_generic_nc3": check_focal_generic,
    "focal_rows": check_focal_rows,
    "focal_edges": check_focal_edges,
    "noncontiguous": check_noncontiguous,
    "refusals": check_refusals,
    "dice_loss": check_dice_loss,
}


# ---- GPU only: the grid-stride loops wrap around ---------------------------------------------------------------------------------------------
# The forward grid is capped at ICL_LOSS_MAX_BLOCKS = 1024 blocks (262,144 voxels per sweep), the backward grid at 4,096 (1,048,576).
FWD_SHAPE = (2, 2, 64, 64, 33)        # 270,336 voxels
BWD_SHAPE = (1, 2, 104, 104, 100)     # 1,081,600 voxels

# N: the error of the plain torch fp32 evaluation of the same formula (the ref_* functions above fed fp32, on the device) against the fp64
# restatement at that shape — value: |v - ref| / |ref|, gradient: max|g - ref| / max|ref| — measured on an MI355X with
# `python tools/point_loss_probe.py --band` (profiles/point_losses.md).  The checks assert <= 2 N, the factor the project gives two
# fp32-grade evaluations.
LARGE_N = {
    "fwd.kl": {"value": 1.5210e-07, "grad0": 2.9974e-07, "grad1": 3.6871e-07},
    "fwd.entropy": {"value": 3.2766e-08, "grad0": 6.0828e-07},
    "fwd.focal": {"value": 8.9297e-08, "grad0": 2.2553e-07},
    "bwd.kl": {"value": 2.5531e-08, "grad0": 3.3384e-07, "grad1": 3.6514e-07},
    "bwd.entropy": {"value": 2.1555e-08, "grad0": 6.0178e-07},
    "bwd.focal": {"value": 5.0026e-08, "grad0": 2.3777e-07},
}


def large_cases(shape):
    nc = shape[1]
    a, b = logits(shape, 901), logits(shape, 902)
    y = synthetic_labels((shape[0],) + tuple(shape[2:]), 903, nc)
    return {
        "kl": (lambda u, v: ops.softmax_kl(u, v, 0.5, 0.5), lambda u, v: ref_kl(u, v, 0.5, 0.5), [a, b], (True, True)),
        "entropy": (lambda u: ops.entropy(u, from_logits=True), lambda u: ref_entropy(u, True), [a], (True,)),
        "focal": (lambda u, t: ops.focal_loss(u, t, 1.5, torch.tensor([0.25, 0.75])), lambda u, t: ref_focal(u, t, 1.5, [0.25, 0.75]),
                  [a, y], (True, False)),
    }


def large_errors(which, mode, dev):
    """(errors of the kernels, errors of torch fp32) against the fp64 restatement on ``dev``, each a dict value / grad0 / grad1."""
    shape = FWD_SHAPE if which == "fwd" else BWD_SHAPE
    fn, ref, tensors, needs = large_cases(shape)[mode]
    want = evaluate(ref, tensors, needs, dev, dtype=torch.float64)
    out = []
    for f in (fn, ref):
        got = evaluate(f, tensors, needs, dev)
        v = float((got[0][0].double() - want[0][0]).abs() / want[0][0].abs())
        d = {"value": v}
        for i, (g, w) in enumerate(zip(got[1], want[1])):
            if w is not None:
                d[f"grad{i}"] = float((g.double() - w).abs().max() / w.abs().max())
        out.append(d)
    return out


def check_large(which, mode, dev):
    mine, _ = large_errors(which, mode, dev)
    n = LARGE_N[f"{which}.{mode}"]
    ok = []
    for k, e in mine.items():
        print(f"{which} {mode} {k}: err {e:.3e}  N {n[k]:.3e}  (asserted <= 2 N)")
        ok.append(e <= 2.0 * n[k])
    assert all(ok), (which, mode, mine, n)


GPU_CHECKS = {f"wrap_{which}_{mode}": (lambda dev, which=which, mode=mode: check_large(which, mode, dev))
              for which in ("fwd", "bwd") for mode in ("kl", "entropy", "focal")}
