"""Shared inputs and checks of the sliding-window kernel tests (tests/test_window_emu.py on the CPU emulator, tests/test_gpu_window.py on
the GPU; icl_amd/csrc/kernels/window.h).  Not a test module.

``torch_loop`` restates the validation loop in torch for a given dtype: pad, walk ``_scan_starts`` at overlap 0.25, optional soft-max,
accumulate with an optional importance map, divide, arg-max, crop.  The predictor is network-free: on a volume from
``hashfill.synthetic_volume(shape, 5)``, window k of the case (counted over its batches, in the loop's order), class c is

    a_c w + b_c w^2 + 0.1 k roll(w, 1, last axis) a_{C-1-c},     a_c = 3 sin(1.7 c + 0.3),  b_c = 2 cos(2.3 c + 0.1)

so the result depends on every window's content, on its place in the walk and on the class order, not on the batch size.  Every reference is computed once
per (case, batch size, form, mode, dtype) and shared.
"""
import functools

import torch
import torch.nn.functional as F

from icl_amd import ops
from icl_amd.utils.hashfill import synthetic_volume
from icl_amd.val_3D import _scan_starts

# (volume, window, classes): what each exercises is said in the test modules
CASES = [
    ((13, 12, 19), (8, 12, 8), 3),      # 2 x 1 x 3 grid, shifted-back last window, origins 5 and 11 off any 16-byte alignment
    ((9, 11, 10), (6, 5, 7), 2),        # 12 windows, rows of 7 (no quad form), three batches of 4 with overlaps inside a batch
    ((5, 12, 6), (8, 12, 8), 16),       # volume smaller than the window on two axes: zero fill in the gather, crop in the finalize
    ((13, 12, 19), (8, 12, 8), 17),     # the class axis walked in memory (C > 16)
    # three more, so that every instantiation of the kernels is reached: origins 0, 12, 16 along a last axis of 32 are all
    # multiples of 4 (quad forms of accumulate and finalize at C <= 4 and at C > 16); 9 classes in the scalar form.  18 classes and not
    # 17 on the small volume: at 17 two of its 768 voxels have a float64 top-two gap below 1e-5, more than the soft-max check admits
    ((6, 4, 32), (4, 4, 16), 3),
    ((6, 4, 32), (4, 4, 16), 18),
    ((5, 6, 7), (4, 4, 5), 9),
]
IDS = [f"{'x'.join(map(str, v))}-{'x'.join(map(str, r))}-C{c}" for v, r, c in CASES]


def gaussian_map(roi, sigma_scale=0.125):
    """The Gaussian window weights, written out independently of icl_amd.val_3D.gaussian_importance_map: float64 per axis, product, / max, fp32,
    floor 1e-3."""
    m = torch.ones((), dtype=torch.float64)
    for r in roi:
        i = torch.arange(r, dtype=torch.float64)
        g = torch.exp(-(i - r // 2) ** 2 / (2 * (sigma_scale * r) ** 2))
        m = m.unsqueeze(-1) * g
    m = m / m.max()
    return m.to(torch.float32).clamp(min=1e-3)


def plan(shape, roi):
    """(pads, padded extent, window origins in the padded frame, in the loop's order)."""
    pads = [(max(r - s, 0) // 2, max(r - s, 0) - max(r - s, 0) // 2) for s, r in zip(shape, roi)]
    psize = [s + a + b for s, (a, b) in zip(shape, pads)]
    grids = [_scan_starts(s, r, 0.25) for s, r in zip(psize, roi)]
    return pads, psize, [(z, y, x) for z in grids[0] for y in grids[1] for x in grids[2]]


def predictor(win, num_classes, k0=0):
    """win [n, 1, r0, r1, r2], windows k0 .. k0 + n - 1 of the case -> [n, C, r0, r1, r2] in win's dtype."""
    c = torch.arange(num_classes, dtype=torch.float64)
    a = (3 * torch.sin(1.7 * c + 0.3)).to(win.dtype).to(win.device).view(1, -1, 1, 1, 1)
    b = (2 * torch.cos(2.3 * c + 0.1)).to(win.dtype).to(win.device).view(1, -1, 1, 1, 1)
    k = torch.arange(k0, k0 + win.shape[0], dtype=win.dtype, device=win.device).view(-1, 1, 1, 1, 1)
    return a * win + b * win * win + 0.1 * k * torch.roll(win, 1, -1) * a.flip(1)


class CountingPredictor:
    """``predictor`` as a callable for the host loops: counts the windows it has been given."""

    def __init__(self, num_classes):
        self.num_classes, self.seen = num_classes, 0

    def __call__(self, win):
        out = predictor(win, self.num_classes, self.seen)
        self.seen += win.shape[0]
        return out


@functools.lru_cache(maxsize=None)
def volume(shape):
    return synthetic_volume(shape, 5).reshape(shape).contiguous()


@functools.lru_cache(maxsize=None)
def torch_loop(case, sw_batch, softmax, gaussian, dtype):
    """The loop in torch, everything in ``dtype`` (the importance map is the fp32 map cast to it).  Returns a dict: score / weight (padded
    maps), quot (cropped quotients), label (cropped arg-max)."""
    shape, roi, nc = CASES[case]
    pads, psize, starts = plan(shape, roi)
    vol = F.pad(volume(shape).to(dtype), [v for a, b in reversed(pads) for v in (a, b)])
    imp = gaussian_map(roi).to(dtype) if gaussian else None
    score = torch.zeros((nc, *psize), dtype=dtype)
    weight = torch.zeros(psize, dtype=dtype)
    for i in range(0, len(starts), sw_batch):
        chunk = starts[i:i + sw_batch]
        win = torch.stack([vol[z:z + roi[0], y:y + roi[1], x:x + roi[2]] for z, y, x in chunk]).unsqueeze(1).contiguous()
        val = predictor(win, nc, i)
        if softmax:
            val = torch.softmax(val, dim=1)
        for j, (z, y, x) in enumerate(chunk):
            if imp is None:
                score[:, z:z + roi[0], y:y + roi[1], x:x + roi[2]] += val[j]
                weight[z:z + roi[0], y:y + roi[1], x:x + roi[2]] += 1
            else:
                score[:, z:z + roi[0], y:y + roi[1], x:x + roi[2]] += val[j] * imp      # the product is rounded, then added
                weight[z:z + roi[0], y:y + roi[1], x:x + roi[2]] += imp
    quot = score / weight
    sl = tuple(slice(a, a + s) for (a, _), s in zip(pads, shape))
    return {"score": score, "weight": weight, "quot": quot[(slice(None),) + sl].contiguous(),
            "label": torch.argmax(quot, dim=0)[sl].contiguous()}


def kernel_loop(case, sw_batch, softmax, gaussian, device):
    """The same loop through ops.window_gather / window_accumulate / window_finalize on ``device`` (fp32); the gathered windows of every
    batch are checked against pad + slice + stack on the way.  Returns the dict of ``torch_loop`` (on the host)."""
    shape, roi, nc = CASES[case]
    pads, psize, starts = plan(shape, roi)
    a = [p[0] for p in pads]
    vol = volume(shape).to(device)
    padded = F.pad(volume(shape), [v for p, q in reversed(pads) for v in (p, q)])
    imp = gaussian_map(roi).to(device) if gaussian else None
    score = torch.zeros((nc, *psize), dtype=torch.float32, device=device)
    weight = torch.zeros(psize, dtype=torch.float32, device=device)
    for i in range(0, len(starts), sw_batch):
        chunk = starts[i:i + sw_batch]
        win = ops.window_gather(vol.unsqueeze(0), chunk, roi, a, psize)
        want = torch.stack([padded[z:z + roi[0], y:y + roi[1], x:x + roi[2]] for z, y, x in chunk]).unsqueeze(1)
        assert torch.equal(win.cpu(), want), ("gather", chunk)
        ops.window_accumulate(predictor(win, nc, i), chunk, score, weight, imp, softmax=softmax)
    score_before = score.clone()
    label, quot = ops.window_finalize(score, weight, a, shape, return_score=True)
    label_only = ops.window_finalize(score_before, weight, a, shape)
    assert torch.equal(label_only, label)
    if list(psize) == list(shape):
        assert quot.data_ptr() == score.data_ptr()      # nothing cropped: divided in place
    return {"score": score_before.cpu(), "weight": weight.cpu(), "quot": quot.cpu(), "label": label.cpu()}


def check_logits_form(case, sw_batch, gaussian, device):
    """Logits form: score map, weight map, quotients and label map EQUAL the fp32 torch loop's (the same adds in the same order, the
    product `w * value` rounded before the add, IEEE division)."""
    want = torch_loop(case, sw_batch, False, gaussian, torch.float32)
    got = kernel_loop(case, sw_batch, False, gaussian, device)
    for k in ("weight", "score", "quot", "label"):
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
        assert torch.equal(got[k], want[k]), (k, (got[k].double() - want[k].double()).abs().max().item())


def check_softmax_form(case, sw_batch, gaussian, device):
    """Soft-max form against the float64 evaluation: the kernels' quotients are at most twice as far from it as the fp32 torch loop's are
    (both distances measured here, on the same input; the factor 2 allows for a different expf), and the labels equal the float64 arg-max
    wherever its top-two gap exceeds 1e-5; at most 1e-3 of the voxels may be left out by that gap (a condition on the inputs)."""
    ref = torch_loop(case, sw_batch, True, gaussian, torch.float64)
    f32 = torch_loop(case, sw_batch, True, gaussian, torch.float32)
    got = kernel_loop(case, sw_batch, True, gaussian, device)
    d_torch = (f32["quot"].double() - ref["quot"]).abs().max().item()
    d_kernel = (got["quot"].double() - ref["quot"]).abs().max().item()
    print(f"softmax form {IDS[case]} sw {sw_batch} gaussian {gaussian}: |fp32 torch - fp64| {d_torch:.3e}, |kernels - fp64| {d_kernel:.3e}")
    assert d_kernel <= 2 * d_torch, (d_kernel, d_torch)
    nc = ref["quot"].shape[0]
    top = torch.topk(ref["quot"], 2, dim=0).values if nc > 1 else None
    clear = (top[0] - top[1]) > 1e-5 if nc > 1 else torch.ones_like(ref["label"], dtype=torch.bool)
    left_out = 1.0 - clear.double().mean().item()
    print(f"    voxels with a float64 top-two gap <= 1e-5: {left_out:.3e}")
    assert left_out <= 1e-3, left_out
    assert torch.equal(got["label"][clear], ref["label"][clear])
    assert torch.equal(got["weight"], f32["weight"])      # the weights never see the soft-max: equal


def check_gather_two_channels(device):
    """Cin = 2, windows hanging over every face of the volume."""
    shape, roi = (5, 7, 6), (4, 8, 4)
    vol = torch.stack([volume(shape), volume(shape).flip(0) * 2 + 1])
    pads, psize = [(1, 2), (1, 0), (2, 3)], [8, 8, 11]
    origins = [(0, 0, 0), (4, 0, 7), (2, 0, 3), (1, 0, 4), (3, 0, 1)]
    padded = F.pad(vol, [v for p, q in reversed(pads) for v in (p, q)])
    got = ops.window_gather(vol.to(device), origins, roi, [p[0] for p in pads], psize)
    want = torch.stack([padded[:, z:z + roi[0], y:y + roi[1], x:x + roi[2]] for z, y, x in origins])
    assert torch.equal(got.cpu(), want)


def check_ties(device):
    """An all-zero score gives label 0 everywhere; two equal classes resolve to the lower index; a NaN wins as in torch.argmax."""
    shape = (3, 4, 8)
    weight = torch.full(shape, 2.0, device=device)
    assert not ops.window_finalize(torch.zeros((5, *shape), device=device), weight, (0, 0, 0), shape).any()
    score = torch.zeros((4, *shape))
    score[1] = 3.0
    score[3] = 3.0
    score[2, 0] = 5.0
    score[3, 1, 2] = float("nan")
    score[1, 2, 3, 5] = float("nan")
    score[2, 2, 3, 5] = float("nan")
    label = ops.window_finalize(score.to(device), weight, (0, 0, 0), shape).cpu()
    assert torch.equal(label, torch.argmax(score / 2.0, dim=0))
    assert label[1, 0, 0] == 1 and label[0, 0, 0] == 2 and label[1, 2, 0] == 3 and label[2, 3, 5] == 1

