"""Shared reference and checks of mirror test-time augmentation in the sliding-window kernels (tests/test_window_tta_emu.py on the CPU
emulator, tests/test_gpu_window_tta.py on the GPU; icl_amd/csrc/kernels/window.h, ``flips=`` of ``ops.window_gather`` /
``ops.window_accumulate``, ``mirror_axes=`` of ``icl_amd.val_3D``).  Not a test module.

The definition, restated in ``torch_loop``: the masks are all subsets of ``mirror_axes`` as integers (bit a = axis a), in increasing
order; a pass is a (window, mask) pair, window-major and mask-minor; a pass predicts ``flip(win, axes)`` and adds ``flip(value, axes)``
— times the importance map, which is NOT flipped — to the score map, and 1 or the importance map to the weight map.  Cases, volumes,
window grid and predictor are those of tests/window_ref.py; the predictor's ``k`` is the index of the PASS, and its ``torch.roll`` makes it
not mirror-equivariant, so a wrong flip, a flipped importance map or a wrong pass order changes the result.
"""
import functools
import itertools

import torch
import torch.nn.functional as F

import window_ref as wr
from icl_amd import ops

CASES, IDS = wr.CASES, wr.IDS
MIRROR_AXES = ((2,), (0, 1), (0, 1, 2))
# The soft-max form's condition on its inputs: at most 1e-3 of the voxels may have a float64 top-two gap <= 1e-5.  Under the pass-indexed
# predictor three (case, mirror_axes) pairs break it — the three-class and two-class cases under all eight mirrors, with 9.4e-3 / 9.8e-3
# (constant / Gaussian), 1.9e-2 / 2.0e-2 and 1.2e-2 / 1.2e-2 of their voxels (measured on the float64 torch loop alone, on the CPU:
# test_window_tta_emu.py::test_softmax_inputs_have_clear_maxima prints every figure) — and are left out of the soft-max checks; the
# others leave out at most 3.4e-4.  Each class layout (C <= 4, <= 16, > 16) keeps cases, and the logits form runs all of them.
SOFTMAX_LEFT_OUT = {(0, (0, 1, 2)), (1, (0, 1, 2)), (4, (0, 1, 2))}


def masks_of(mirror_axes):
    return sorted(sum(1 << a for a in sub) for n in range(len(mirror_axes) + 1) for sub in itertools.combinations(mirror_axes, n))


def dims_of(mask, first):
    return [first + a for a in range(3) if mask >> a & 1]


def pad_volume(vol, pads):
    return F.pad(vol, [v for a, b in reversed(pads) for v in (a, b)])


def loop(vol, roi, nc, pads, starts, mirror_axes, per_forward, softmax, imp, predict, dtype):
    """The loop of the definition in torch, everything in ``dtype``.  vol [s0, s1, s2] unpadded; ``mirror_axes`` None: one pass per window,
    nothing flipped.  ``predict(win, k0)`` -> [n, C, *roi].  Returns score / weight (padded), quot / label (cropped)."""
    shape = tuple(vol.shape)
    psize = [s + a + b for s, (a, b) in zip(shape, pads)]
    vol = pad_volume(vol.to(dtype), pads)
    imp = None if imp is None else imp.to(dtype)
    passes = [(o, f) for o in starts for f in (masks_of(mirror_axes) if mirror_axes is not None else [0])]
    score = torch.zeros((nc, *psize), dtype=dtype)
    weight = torch.zeros(psize, dtype=dtype)
    for i in range(0, len(passes), per_forward):
        chunk = passes[i:i + per_forward]
        win = torch.stack([torch.flip(vol[z:z + roi[0], y:y + roi[1], x:x + roi[2]], dims_of(f, 0)) for (z, y, x), f in chunk]).unsqueeze(1)
        val = predict(win.contiguous(), i)
        val = torch.softmax(val, dim=1) if softmax else val.to(dtype)
        for j, ((z, y, x), f) in enumerate(chunk):
            back = torch.flip(val[j], dims_of(f, 1))
            if imp is None:
                score[:, z:z + roi[0], y:y + roi[1], x:x + roi[2]] += back
                weight[z:z + roi[0], y:y + roi[1], x:x + roi[2]] += 1
            else:
                score[:, z:z + roi[0], y:y + roi[1], x:x + roi[2]] += back * imp      # the product is rounded, then added; imp is not flipped
                weight[z:z + roi[0], y:y + roi[1], x:x + roi[2]] += imp
    quot = score / weight
    sl = tuple(slice(a, a + s) for (a, _), s in zip(pads, shape))
    return {"score": score, "weight": weight, "quot": quot[(slice(None),) + sl].contiguous(), "label": torch.argmax(quot, dim=0)[sl].contiguous()}


@functools.lru_cache(maxsize=None)
def torch_loop(case, mirror_axes, per_forward, softmax, gaussian, dtype):
    shape, roi, nc = CASES[case]
    pads, _, starts = wr.plan(shape, roi)
    return loop(wr.volume(shape), roi, nc, pads, starts, mirror_axes, per_forward, softmax, wr.gaussian_map(roi) if gaussian else None,
                lambda win, k: wr.predictor(win, nc, k), dtype)


def kernel_loop(case, mirror_axes, per_forward, softmax, gaussian, device, predict=None):
    """The same loop through ``ops.window_gather(flips=)`` / ``window_accumulate(flips=)`` / ``window_finalize`` on ``device``; every
    gathered batch is checked against torch.flip of pad + slice + stack on the way."""
    shape, roi, nc = CASES[case]
    pads, psize, starts = wr.plan(shape, roi)
    a = [p[0] for p in pads]
    vol = wr.volume(shape).to(device)
    padded = pad_volume(wr.volume(shape), pads)
    imp = wr.gaussian_map(roi).to(device) if gaussian else None
    predict = predict or (lambda win, k: wr.predictor(win, nc, k))
    passes = [(o, f) for o in starts for f in (masks_of(mirror_axes) if mirror_axes is not None else [None])]
    score = torch.zeros((nc, *psize), dtype=torch.float32, device=device)
    weight = torch.zeros(psize, dtype=torch.float32, device=device)
    for i in range(0, len(passes), per_forward):
        chunk = passes[i:i + per_forward]
        origins = [o for o, _ in chunk]
        flips = None if mirror_axes is None else [f for _, f in chunk]
        win = ops.window_gather(vol.unsqueeze(0), origins, roi, a, psize, flips=flips)
        want = torch.stack([torch.flip(padded[z:z + roi[0], y:y + roi[1], x:x + roi[2]], dims_of(f or 0, 0)) for (z, y, x), f in chunk])
        assert torch.equal(win.cpu(), want.unsqueeze(1)), ("gather", chunk)
        ops.window_accumulate(predict(win, i), origins, score, weight, imp, softmax=softmax, flips=flips)
    label, quot = ops.window_finalize(score.clone(), weight, a, shape, return_score=True)
    return {"score": score.cpu(), "weight": weight.cpu(), "quot": quot.cpu(), "label": label.cpu()}


# ---- 1. gather ---------------------------------------------------------------------------------------------------------------------------

def check_gather(case, device):
    """Every origin of the case under each of the 8 masks (one mask per launch), then 8 different masks on one origin in one launch."""
    shape, roi, _ = CASES[case]
    pads, psize, starts = wr.plan(shape, roi)
    a = [p[0] for p in pads]
    vol = wr.volume(shape).to(device).unsqueeze(0)
    padded = pad_volume(wr.volume(shape), pads)

    def window(o, f):
        return torch.flip(padded[o[0]:o[0] + roi[0], o[1]:o[1] + roi[1], o[2]:o[2] + roi[2]], dims_of(f, 0))
    for f in range(8):
        got = ops.window_gather(vol, starts, roi, a, psize, flips=[f] * len(starts))
        assert torch.equal(got.cpu(), torch.stack([window(o, f) for o in starts]).unsqueeze(1)), f
    for o in (starts[0], starts[-1]):
        order = [5, 0, 7, 2, 1, 6, 3, 4]
        got = ops.window_gather(vol, [o] * 8, roi, a, psize, flips=order)
        assert torch.equal(got.cpu(), torch.stack([window(o, f) for f in order]).unsqueeze(1)), o


def check_gather_two_channels(device):
    """Cin = 2, windows hanging over every face of the volume, a different mask each (wr.check_gather_two_channels' geometry)."""
    shape, roi = (5, 7, 6), (4, 8, 4)
    vol = torch.stack([wr.volume(shape), wr.volume(shape).flip(0) * 2 + 1])
    pads, psize = [(1, 2), (1, 0), (2, 3)], [8, 8, 11]
    origins = [(0, 0, 0), (4, 0, 7), (2, 0, 3), (1, 0, 4), (3, 0, 1), (4, 0, 7), (0, 0, 0), (2, 0, 3)]
    flips = [7, 4, 1, 2, 6, 3, 5, 0]
    padded = pad_volume(vol, pads)
    got = ops.window_gather(vol.to(device), origins, roi, [p[0] for p in pads], psize, flips=flips)
    want = torch.stack([torch.flip(padded[:, z:z + roi[0], y:y + roi[1], x:x + roi[2]], dims_of(f, 1)) for (z, y, x), f in zip(origins, flips)])
    assert torch.equal(got.cpu(), want)


# ---- 2. / 3. the two forms ------------------------------------------------------------------------------------------------------------------

def check_logits_form(case, mirror_axes, per_forward, gaussian, device):
    """Score map, weight map, quotients and labels EQUAL the fp32 torch loop's."""
    want = torch_loop(case, mirror_axes, per_forward, False, gaussian, torch.float32)
    got = kernel_loop(case, mirror_axes, per_forward, False, gaussian, device)
    for k in ("weight", "score", "quot", "label"):
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
        assert torch.equal(got[k], want[k]), (k, (got[k].double() - want[k].double()).abs().max().item())


def clear_maxima(ref):
    """(mask of the voxels whose float64 top-two gap exceeds 1e-5, the share of the others)."""
    top = torch.topk(ref["quot"], 2, dim=0).values
    clear = (top[0] - top[1]) > 1e-5
    return clear, 1.0 - clear.double().mean().item()


def softmax_bound(got_quot, got_label, case, mirror_axes, per_forward, gaussian, what):
    """The rule of ``window_ref.check_softmax_form`` for quotients and labels computed some way (``what``) on the case."""
    ref = torch_loop(case, mirror_axes, per_forward, True, gaussian, torch.float64)
    f32 = torch_loop(case, mirror_axes, per_forward, True, gaussian, torch.float32)
    d_torch = (f32["quot"].double() - ref["quot"]).abs().max().item()
    d_got = (got_quot.double() - ref["quot"]).abs().max().item()
    print(f"softmax form {IDS[case]} axes {mirror_axes} per forward {per_forward} gaussian {gaussian}: |fp32 torch - fp64| {d_torch:.3e}, "
          f"|{what} - fp64| {d_got:.3e}")
    assert d_got <= 2 * d_torch, (d_got, d_torch)
    clear, left_out = clear_maxima(ref)
    print(f"    voxels with a float64 top-two gap <= 1e-5: {left_out:.3e}")
    assert left_out <= 1e-3, left_out
    assert torch.equal(got_label[clear], ref["label"][clear])
    return f32


def check_softmax_form(case, mirror_axes, per_forward, gaussian, device):
    got = kernel_loop(case, mirror_axes, per_forward, True, gaussian, device)
    f32 = softmax_bound(got["quot"], got["label"], case, mirror_axes, per_forward, gaussian, "kernels")
    assert torch.equal(got["weight"], f32["weight"])      # the weights never see the soft-max: equal


# ---- 6. a mirror-equivariant predictor -----------------------------------------------------------------------------------------------------

def pointwise(nc):
    """``window_ref.predictor`` without its roll and without the pass index: point-wise, hence equivariant under every mirror."""
    c = torch.arange(nc, dtype=torch.float64)
    a, b = (3 * torch.sin(1.7 * c + 0.3)).float().view(1, -1, 1, 1, 1), (2 * torch.cos(2.3 * c + 0.1)).float().view(1, -1, 1, 1, 1)
    return lambda win, k: a.to(win.device) * win + b.to(win.device) * win * win


def check_equivariant(case, device):
    """Point-wise predictor, constant weights, logits form: every pass over a voxel adds the same value, so TTA and no TTA give the same
    labels, and quotients that agree to a relative (N_tta + N_plain + 2) 2^-24 — the sequential fp32 sums of N equal terms ((N - 1) 2^-24
    each) and the two divisions; N, the most passes over a voxel, is read off the weight maps."""
    nc = CASES[case][2]
    plain = kernel_loop(case, None, 4, False, False, device, pointwise(nc))
    tta = kernel_loop(case, (0, 1, 2), 16, False, False, device, pointwise(nc))
    n_plain, n_tta = int(plain["weight"].max().item()), int(tta["weight"].max().item())
    assert n_tta == 8 * n_plain
    bound = (n_tta + n_plain + 2) * 2.0 ** -24
    rel = ((tta["quot"].double() - plain["quot"].double()).abs() / plain["quot"].double().abs().clamp(min=1e-300)).max().item()
    print(f"equivariant {IDS[case]}: N_tta {n_tta}, N_plain {n_plain}, largest relative difference {rel:.3e}, bound {bound:.3e}")
    assert ((tta["quot"].double() - plain["quot"].double()).abs() <= bound * plain["quot"].double().abs()).all()
    assert torch.equal(tta["label"], plain["label"])


# ---- 5. predictors of the host loops -------------------------------------------------------------------------------------------------------

class PredictorNet(torch.nn.Module):
    """``window_ref.predictor`` as the ``nn.Module`` that ``test_single_case_base`` wants: one dummy parameter (it places the module on a
    device), the count of the samples seen as the pass index; ``dtype`` casts the output (fp16: the BraTS loop's kernels hand over)."""

    def __init__(self, num_classes, device="cpu", dtype=None):
        super().__init__()
        self.dummy = torch.nn.Parameter(torch.zeros(1, device=device), requires_grad=False)
        self.num_classes, self.dtype, self.seen, self.calls = num_classes, dtype, 0, 0

    def forward(self, win):
        out = wr.predictor(win, self.num_classes, self.seen)
        self.seen += win.shape[0]
        self.calls += 1
        return out if self.dtype is None else out.to(self.dtype)


AMOS_SHAPE, AMOS_CLASSES, AMOS_AXES = CASES[2][0], 3, (0, 1, 2)


@functools.lru_cache(maxsize=None)
def amos_label():
    """The label map that ``test_all_case_amos(mirror_axes=AMOS_AXES)`` scores for the volume of AMOS_SHAPE: its window is 96^3, so the small
    volume is zero-padded into ONE window, whose 8 mirrors are the passes (4 per forward, constant weights, logits form)."""
    pads = [((96 - s) // 2, 96 - s - (96 - s) // 2) for s in AMOS_SHAPE]
    return loop(wr.volume(AMOS_SHAPE), (96, 96, 96), AMOS_CLASSES, pads, [(0, 0, 0)], AMOS_AXES, 4, False, None,
                lambda win, k: wr.predictor(win, AMOS_CLASSES, k), torch.float32)["label"]
