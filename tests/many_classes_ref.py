"""Shared checks of the 17 .. 256 class training kernels (tests/test_many_classes_emu.py on the kernel emulation,
tests/test_gpu_many_classes.py on the device): the fused losses against torch-CPU functional ops, as test_fused_losses states them, and
the prototype attention against the torch restatement of test_prototype_attention.  Every check runs its calls twice and asks the two
runs to agree bit for bit (the generic-class kernels sum per-block partials in a fixed order: no float atomics).

Bands (the project's own, tests/test_kernels_emu.py): loss values abs < 1e-5 (MSE < 1e-6), gradients rel_err < 1e-4; attention outputs and
logits 1e-5, gradients 1e-4.  torch fp32 itself is within 1e-6 (values) and 2e-7 (gradients) of torch fp64 at these shapes.
"""
import torch
import torch.nn.functional as F

from conftest import rel_err
from icl_amd import ops
from icl_amd.utils.hashfill import synthetic_labels, synthetic_volume

LOSS_CASES = [(17, (6, 5, 7), 1.0), (32, (6, 5, 7), 1.0), (40, (6, 5, 7), 1.0), (256, (6, 5, 7), 1.0),      # fewer voxels than a block
              (17, (24, 24, 24), 1.0),      # several blocks write partials
              (17, (6, 5, 7), 30.0)]        # saturated soft-max
ATTN_CASES = [(2, 2, 17, 8, 70), (1, 4, 40, 16, 300), (1, 1, 256, 16, 64), (1, 2, 17, 16, 4200)]
ATTN_SMALL_CASES = [(2, 2, 3, 8, 70), (1, 4, 2, 16, 300), (1, 1, 16, 16, 64)]      # of test_prototype_attention: one class tile


def rand(shape, seed):
    return synthetic_volume(tuple(shape), seed)


def _hard_dice_ref(p, lab, nc, w=None):
    d = 0
    for c in range(nc):
        t = (lab == c).float()
        d = d + (w[c] if w else 1.0) * (1 - (2 * (p[:, c] * t).sum() + 1e-5) / ((p[:, c] ** 2).sum() + t.sum() + 1e-5))
    return d / nc


def _soft_dice_ref(sa, sb, nc):
    d = 0
    for c in range(nc):
        d = d + (1 - (2 * (sa[:, c] * sb[:, c]).sum() + 1e-5) / (sa[:, c].sum() + sb[:, c].sum() + 1e-5))
    return d / nc


def loss_inputs(nc, S, scale, B=2):
    lab = synthetic_labels((B,) + tuple(S), 31, nc)
    return dict(lab=lab, a=rand((B, nc) + tuple(S), 32) * 2 * scale, p=torch.softmax(rand((B, nc) + tuple(S), 33) * scale, 1),
                b=rand((B, nc) + tuple(S), 34) * 2 * scale, a2=rand((B, nc) + tuple(S), 35) * 2 * scale,
                w=[0.5 + 0.1 * (i % 7) for i in range(nc)])


_REF = {}


def loss_reference(nc, S, scale):
    """torch-CPU values and gradients of the four terms, computed once per case and shared."""
    key = (nc, tuple(S), scale)
    if key in _REF:
        return _REF[key]
    x = loss_inputs(nc, S, scale)
    lab = x["lab"]
    ar = x["a"].clone().requires_grad_()
    cr, dr = F.cross_entropy(ar, lab), _hard_dice_ref(torch.softmax(ar, 1), lab, nc)
    (1.3 * cr + 0.7 * dr).backward()
    pr = x["p"].clone().requires_grad_()
    wd = _hard_dice_ref(pr, lab, nc, x["w"])
    wd.backward()
    a2r = x["a2"].clone().requires_grad_()
    sa, sb = torch.softmax(a2r, 1), torch.softmax(x["b"], 1)
    sdr, msr = _soft_dice_ref(sa, sb, nc), ((sa - sb) ** 2).mean()
    (sdr + 10 * msr).backward()
    _REF[key] = dict(ce=float(cr), dice=float(dr), ga=ar.grad, wdice=float(wd), gp=pr.grad, sdice=float(sdr), mse=float(msr), ga2=a2r.grad)
    return _REF[key]


def run_losses(nc, S, scale, dev):
    """The four terms through the wrappers on ``dev``: values as floats, gradients on the CPU."""
    x = loss_inputs(nc, S, scale)
    lab = x["lab"].to(dev)
    a = x["a"].to(dev).requires_grad_()
    ce, dc = ops.cross_entropy_dice_parts(a, lab, nc)
    (1.3 * ce + 0.7 * dc).backward()
    p = x["p"].to(dev).requires_grad_()
    wd = ops.dice_loss(p, lab, nc, softmax=False, weight=x["w"])
    wd.backward()
    b = x["b"].to(dev)
    a2 = x["a2"].to(dev).requires_grad_()
    sd, ms = ops.soft_dice_loss(a2, b), ops.softmax_mse(a2, b)
    (sd + 10 * ms).backward()
    return dict(ce=float(ce.detach()), dice=float(dc.detach()), ga=a.grad.cpu(), wdice=float(wd.detach()), gp=p.grad.cpu(),
                sdice=float(sd.detach()), mse=float(ms.detach()),
                ga2=a2.grad.cpu())


VALUE_BANDS = dict(ce=1e-5, dice=1e-5, wdice=1e-5, sdice=1e-5, mse=1e-6)
GRADS = ("ga", "gp", "ga2")


def assert_losses_close(got, ref, what):
    for k, band in VALUE_BANDS.items():
        print(f"{what} {k}: {got[k]:.8f} vs {ref[k]:.8f} (|diff| {abs(got[k] - ref[k]):.2e}, band {band:g})")
    for k in GRADS:
        print(f"{what} {k}: rel_err {rel_err(got[k], ref[k]):.2e} (band 1e-4)")
    for k, band in VALUE_BANDS.items():
        assert abs(got[k] - ref[k]) < band, (what, k, got[k], ref[k])
    for k in GRADS:
        assert rel_err(got[k], ref[k]) < 1e-4, (what, k, rel_err(got[k], ref[k]))


def assert_bit_equal(r1, r2, what):
    for k in VALUE_BANDS:
        assert r1[k] == r2[k], (what, k, r1[k], r2[k])
    for k in GRADS:
        assert torch.equal(r1[k], r2[k]), (what, k)


def check_losses(nc, S, scale, dev):
    r1 = run_losses(nc, S, scale, dev)
    r2 = run_losses(nc, S, scale, dev)
    assert_bit_equal(r1, r2, f"nc={nc} S={S}")
    assert_losses_close(r1, loss_reference(nc, S, scale), f"nc={nc} S={S} x{scale:g}")
    if nc == 256:
        assert len(torch.unique(loss_inputs(nc, S, scale)["lab"])) < nc      # classes absent from the labels: Y_c = 0


def multi_terms(nc, S, dev, B=2):
    """Five terms of the trainer's kinds (CE + Dice, CE + Dice, soft Dice, two soft-max MSE at their own sizes) and their leaves."""
    S = tuple(S)
    lab = synthetic_labels((B,) + S, 31, nc).to(dev)
    mk = lambda shape, seed: rand((B, nc) + tuple(shape), seed).to(dev)      # noqa: E731
    small = (3, 4, 5)
    leaves = [mk(S, 1).requires_grad_(), mk(S, 2).requires_grad_(), mk(S, 3).requires_grad_(), mk(small, 4).requires_grad_(),
              mk(S, 5).requires_grad_()]
    terms = [(leaves[0], lab, 1), (leaves[1], lab, 1), (leaves[2], mk(S, 6), 2), (leaves[3], mk(small, 7), 3), (leaves[4], mk(S, 8), 3)]
    return terms, leaves


def run_multi(nc, S, dev, single):
    """(values, gradients) of multi_terms through ops.fused_losses, or term by term with ``single``."""
    terms, leaves = multi_terms(nc, S, dev)
    if single:
        pairs = [ops._FusedLoss.apply(a, (t.long() if m <= 1 else t.detach()), None, m, False) for a, t, m in terms]
    else:
        pairs = ops.fused_losses(terms)
    modes = [m for _, _, m in terms]
    tot = sum((0.3 + 0.1 * j) * (p[0] if modes[j] in (1, 3) else p[1]) + (0.5 * p[1] if modes[j] == 1 else 0.0) for j, p in enumerate(pairs))
    tot.backward()
    vals = [float(p[0]) if modes[j] == 3 else float(p[1]) for j, p in enumerate(pairs)] + [float(pairs[0][0]), float(pairs[1][0])]
    return vals, [x.grad.cpu() for x in leaves]


def multi_reference(nc, S):
    """torch-CPU statement of run_multi."""
    terms, leaves = multi_terms(nc, S, torch.device("cpu"))
    vals, ces, tot = [], [], 0
    for j, (a, t, m) in enumerate(terms):
        w = 0.3 + 0.1 * j
        if m == 1:
            ce, dc = F.cross_entropy(a, t), _hard_dice_ref(torch.softmax(a, 1), t, nc)
            tot = tot + w * ce + 0.5 * dc
            vals.append(float(dc))
            ces.append(float(ce))
        elif m == 2:
            sd = _soft_dice_ref(torch.softmax(a, 1), torch.softmax(t, 1), nc)
            tot = tot + w * sd
            vals.append(float(sd))
        else:
            ms = ((torch.softmax(a, 1) - torch.softmax(t, 1)) ** 2).mean()
            tot = tot + w * ms
            vals.append(float(ms))
    tot.backward()
    return vals + ces, [x.grad for x in leaves]


MULTI_BANDS = [1e-5, 1e-5, 1e-5, 1e-6, 1e-6, 1e-5, 1e-5]      # Dice, Dice, soft Dice, MSE, MSE, CE, CE


def assert_multi_close(got, ref, what):
    for k, (g, r, band) in enumerate(zip(got[0], ref[0], MULTI_BANDS)):
        print(f"{what} value {k}: |diff| {abs(g - r):.2e} (band {band:g})")
        assert abs(g - r) < band, (what, k, g, r)
    for k, (g, r) in enumerate(zip(got[1], ref[1])):
        print(f"{what} gradient {k}: rel_err {rel_err(g, r):.2e} (band 1e-4)")
        assert rel_err(g, r) < 1e-4, (what, k, rel_err(g, r))


def run_attention(B, h, nc, d, N, dev):
    C = h * d
    qh = rand((B, h, nc, d), 71).to(dev).requires_grad_()
    kv = rand((B, N, 2 * C), 72).to(dev).requires_grad_()
    go, gl = rand((B, h, nc, d), 73).to(dev), rand((B, nc, h, N), 74).to(dev)
    out, logits = ops.prototype_attention(qh, kv, h, d ** -0.5)
    assert logits.shape == (B, nc, h, N) and logits.is_contiguous()
    ((out * go).sum() + (logits * gl).sum()).backward()
    return out.detach().cpu(), logits.detach().cpu(), qh.grad.cpu(), kv.grad.cpu()


_ATTN_REF = {}


def attention_reference(B, h, nc, d, N):
    key = (B, h, nc, d, N)
    if key not in _ATTN_REF:
        C = h * d
        qr, kr = rand((B, h, nc, d), 71).requires_grad_(), rand((B, N, 2 * C), 72).requires_grad_()
        go, gl = rand((B, h, nc, d), 73), rand((B, nc, h, N), 74)
        kvp = kr.reshape(B, N, 2, h, d).permute(2, 0, 3, 1, 4)
        lr4 = (qr @ kvp[0].transpose(-2, -1)) * d ** -0.5
        orf = lr4.softmax(dim=-1) @ kvp[1]
        lr = lr4.permute(0, 2, 1, 3)
        ((orf * go).sum() + (lr * gl).sum()).backward()
        _ATTN_REF[key] = (orf.detach(), lr.detach().contiguous(), qr.grad, kr.grad)
    return _ATTN_REF[key]


def check_attention(B, h, nc, d, N, dev, against=None):
    """Both backward entry points: the wrapper takes icl_attn_bwd_ws with its dQ-share workspace from 1,024 tokens on and the
    row-per-workgroup dQ kernel below; ``ops.PROTO_ATTN_WS_MIN_TOKENS`` moves that threshold, so every case runs both."""
    ref = against or attention_reference(B, h, nc, d, N)
    keep = ops.PROTO_ATTN_WS_MIN_TOKENS
    try:
        for thresh in (1, 1 << 30):
            ops.PROTO_ATTN_WS_MIN_TOKENS = thresh
            got = run_attention(B, h, nc, d, N, dev)
            again = run_attention(B, h, nc, d, N, dev)
            for g, a in zip(got, again):
                assert torch.equal(g, a)
            errs = [rel_err(g, r) for g, r in zip(got, ref)]
            print(f"attention {(B, h, nc, d, N)} ws={'yes' if thresh == 1 else 'no'}: out {errs[0]:.2e} logits {errs[1]:.2e} (band 1e-5), "
                  f"dq {errs[2]:.2e} dkv {errs[3]:.2e} (band 1e-4)")
            assert errs[0] < 1e-5 and errs[1] < 1e-5, errs
            assert errs[2] < 1e-4 and errs[3] < 1e-4, errs
    finally:
        ops.PROTO_ATTN_WS_MIN_TOKENS = keep


# ---------------------------------------------------------------- fixtures of tests/golden/many_classes.npz (make_golden_many_classes.py)
GOLDEN_NC = 17
ALIGNER_GEOM = dict(chans=(64, 32, 16), res=(2, 2, 4), heads=(4, 2, 2), batch=2)
LOGIT_SAMPLES = 2000


def sample_index(numel: int, count: int):
    """``count`` flat indices spread over a tensor of ``numel`` elements by a multiplicative hash (generator and tests agree on them)."""
    import numpy as np
    return ((np.arange(count, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(12345)) % np.uint64(numel)).astype(np.int64)


def aligner_feats():
    g = ALIGNER_GEOM
    return [rand((g["batch"], c, r, r, r), 21 + i) for i, (c, r) in enumerate(zip(g["chans"], g["res"]))]


def aligner_loss(maps, maps_u):
    return sum((m * rand(m.shape, 30 + i).to(m.device)).sum() for i, m in enumerate(maps)) \
        + sum((m * rand(m.shape, 40 + i).to(m.device)).sum() for i, m in enumerate(maps_u))


def check_aligner(dev, g, tag, train):
    """icl_amd's InherentConsistent at 17 classes against the reference's (own-query call, then the guided call with the queries of
    the first), with the bands of the aligner unit golden test (tests/test_oracle_golden.py::test_aligner_matches_reference): outputs
    1e-4, feature-map gradients 1e-3; guided_Q's gradient like the feature maps' element-wise, and its norm to 2e-3 as every parameter
    gradient there.  Above 16 classes the levels take the operator-by-operator path (ops.query_chain_ok)."""
    from icl_amd.networks.aligner import DropPath, InherentConsistent
    from icl_amd.utils.hashfill import fill_like_reference_init
    geo = ALIGNER_GEOM
    ops.StepRNG.tensor = None
    m = InherentConsistent(in_chans=geo["chans"], depths=(2, 2, 2), input_resolution=geo["res"], num_classes=GOLDEN_NC,
                           num_heads=geo["heads"], device=dev)
    fill_like_reference_init(list(m.named_parameters()))
    for mod in m.modules():
        if isinstance(mod, DropPath):
            mod.drop_prob = 0.0
    m.train(train)
    feats = [f.to(dev).requires_grad_() for f in aligner_feats()]
    maps, qs = m(feats, None, "labeled")
    maps_u, qs_u = m(feats, qs, "unlabeled")
    aligner_loss(maps, maps_u).backward()
    for i in range(3):
        for name, t in (("map", maps[i]), ("q", qs[i]), ("mapu", maps_u[i]), ("qu", qs_u[i])):
            e = rel_err(t.detach().cpu(), g[f"al_{tag}_{name}{i}"])
            print(f"aligner {tag} {name}{i}: {e:.2e} (band 1e-4)")
            assert e < 1e-4, (tag, name, i, e)
        e = rel_err(feats[i].grad.cpu(), g[f"al_{tag}_gfeat{i}"])
        print(f"aligner {tag} gfeat{i}: {e:.2e} (band 1e-3)")
        assert e < 1e-3, (tag, i, e)
    gq, ref = m.guided_Q.grad.cpu(), g[f"al_{tag}_g.guided_Q"]
    e = rel_err(gq, ref)
    print(f"aligner {tag} guided_Q gradient: {e:.2e} (band 1e-3)")
    assert e < 1e-3, (tag, e)
    rn = float((ref.astype("float64") ** 2).sum() ** 0.5)
    assert abs(float(gq.double().norm()) - rn) <= 2e-3 * max(rn, 1e-5)
