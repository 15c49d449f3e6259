"""GPU tests of mirror test-time augmentation in the sliding-window kernels (run with -m gpu; icl_amd/csrc/kernels/window.h: the WinFlips
instantiations of ``window_gather_kernel`` and ``window_accumulate_kernel``, launched by ``icl_window_gather_flipped`` /
``icl_window_accumulate_flipped``) and of ``mirror_axes=`` in the two validation loops of ``icl_amd.val_3D``.

The definition, the cases, the reference loop and the assertions are those of tests/test_window_tta_emu.py (tests/window_tta_ref.py):
the gather bit-equal to ``torch.flip`` of pad + slice + stack, the logits form EQUAL to the fp32 torch loop, the soft-max form within the
float64 bound of ``window_ref.check_softmax_form``.  The loops run in their kernel form and, behind ``ICL_VAL_WINDOWS=aten``, in their
ATen form.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import window_ref as wr  # noqa: E402
import window_tta_ref as tr  # noqa: E402
from icl_amd import ops, val_3D  # noqa: E402
from icl_amd.utils.hashfill import synthetic_labels  # noqa: E402

pytestmark = pytest.mark.gpu

CASE_PARAMS = [pytest.param(i, id=tr.IDS[i]) for i in range(len(tr.CASES))]
AXES_PARAMS = [pytest.param(a, id="axes" + "".join(map(str, a))) for a in tr.MIRROR_AXES]
SOFTMAX_PARAMS = [pytest.param(i, a, id=f"{tr.IDS[i]}-axes{''.join(map(str, a))}") for i in range(len(tr.CASES)) for a in tr.MIRROR_AXES
                  if (i, a) not in tr.SOFTMAX_LEFT_OUT]


@pytest.fixture(scope="module")
def dev():
    from icl_amd import _lib
    assert _lib.lib_path().endswith("libicl_hip.so"), "GPU tests must run on the HIP library"
    return torch.device("cuda", 0)


def _both_ways(monkeypatch, fn):
    out = {}
    for way in ("device", "aten"):
        monkeypatch.setenv("ICL_VAL_WINDOWS", way)
        out[way] = fn()
    return out["device"], out["aten"]


# ---- 1. gather ----

@pytest.mark.parametrize("case", CASE_PARAMS)
def test_gather_equals_torch_flip(dev, case):
    tr.check_gather(case, dev)


def test_gather_two_channels(dev):
    tr.check_gather_two_channels(dev)


# ---- 2. logits form ----

@pytest.mark.parametrize("gaussian", [False, True], ids=["constant", "gaussian"])
@pytest.mark.parametrize("per_forward", [1, 4, 16])
@pytest.mark.parametrize("axes", AXES_PARAMS)
@pytest.mark.parametrize("case", CASE_PARAMS)
def test_logits_form_equals_the_fp32_torch_loop(dev, case, axes, per_forward, gaussian):
    tr.check_logits_form(case, axes, per_forward, gaussian, dev)


# ---- 3. soft-max form (the condition on its inputs is checked on the CPU: test_window_tta_emu.py) ----

@pytest.mark.parametrize("gaussian", [False, True], ids=["constant", "gaussian"])
@pytest.mark.parametrize("per_forward", [4, 16])
@pytest.mark.parametrize("case,axes", SOFTMAX_PARAMS)
def test_softmax_form_against_float64(dev, case, axes, per_forward, gaussian):
    tr.check_softmax_form(case, axes, per_forward, gaussian, dev)


# ---- 4. identity ----

@pytest.mark.parametrize("case", [0, 2], ids=[tr.IDS[0], tr.IDS[2]])
def test_empty_mirror_axes_is_no_augmentation(dev, case):
    """``mirror_axes=()``: one pass per window with mask 0 (the WinFlips instantiations) — bit-equal to ``None`` (the plain ones)."""
    shape, roi, nc = tr.CASES[case]
    x = wr.volume(shape)[None, None].to(dev)
    a = val_3D.sliding_window_inference(x, roi, 4, wr.CountingPredictor(nc), mode="gaussian")
    b = val_3D.sliding_window_inference(x, roi, 4, wr.CountingPredictor(nc), mode="gaussian", mirror_axes=())
    assert torch.equal(a, b)
    image = wr.volume(shape).numpy()
    a = val_3D.test_single_case_base(tr.PredictorNet(nc, dev), "unet_3D", image, 6, 6, roi, num_classes=nc, return_score=True)
    b = val_3D.test_single_case_base(tr.PredictorNet(nc, dev), "unet_3D", image, 6, 6, roi, num_classes=nc, return_score=True, mirror_axes=())
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- 5. host loops ----

@pytest.mark.parametrize("gaussian", [False, True], ids=["constant", "gaussian"])
def test_sliding_window_inference_all_mirrors(dev, monkeypatch, gaussian):
    """The predictor sees 8 x windows samples; the kernel form equals the ATen form, and both the reference loop, bit for bit."""
    case = 0
    shape, roi, nc = tr.CASES[case]
    windows = len(wr.plan(shape, roi)[2])
    x = wr.volume(shape)[None, None].to(dev)

    def run():
        pred = wr.CountingPredictor(nc)
        out = val_3D.sliding_window_inference(x, roi, 4, pred, mode="gaussian" if gaussian else "constant", mirror_axes=(0, 1, 2))
        assert pred.seen == 8 * windows
        return out
    got, aten = _both_ways(monkeypatch, run)
    assert torch.equal(got, aten)
    assert torch.equal(got[0].cpu(), tr.torch_loop(case, (0, 1, 2), 4, False, gaussian, torch.float32)["quot"])


def test_hand_over_in_the_middle_of_the_mirrors(dev, monkeypatch):
    """A first prediction that the kernel form does not take — 257 classes in the AMOS loop, fp16 in the BraTS loop — hands over after the
    first batch of PASSES (5 per forward: it ends inside a window's eight mirrors): every pass goes through the predictor once and the
    result is that of ``ICL_VAL_WINDOWS=aten``."""
    case = 0
    shape, roi, nc = tr.CASES[case]
    windows = len(wr.plan(shape, roi)[2])
    x = wr.volume(shape)[None, None].to(dev)

    def amos():
        pred = wr.CountingPredictor(257)
        out = val_3D.sliding_window_inference(x, roi, 5, pred, mode="gaussian", mirror_axes=(0, 1, 2))
        assert pred.seen == 8 * windows
        return out
    got, aten = _both_ways(monkeypatch, amos)
    assert got.shape == (1, 257, *shape) and torch.equal(got, aten)

    def brats():
        net = tr.PredictorNet(nc, dev, torch.float16)
        out = val_3D.test_single_case_base(net, "unet_3D", wr.volume(shape).numpy(), 6, 6, roi, num_classes=nc, windows_per_batch=5,
                                           return_score=True, mode="gaussian", mirror_axes=(0, 1, 2))
        assert net.seen == 8 * windows and net.calls == -(-8 * windows // 5)
        return out
    got, aten = _both_ways(monkeypatch, brats)
    assert np.array_equal(got[0], aten[0]) and np.array_equal(got[1], aten[1])


def test_single_case_base_all_mirrors(dev, monkeypatch):
    """``test_single_case_base(mirror_axes=(0, 1, 2))`` on an ``nn.Module`` around the synthetic predictor; on the last case (8 windows,
    9 classes) strides of 3 give the grid of ``window_ref.plan``.  The two forms go through different ``expf``s, so they are not held to
    equality: the kernel form is held to the soft-max bound against the float64 loop (quotients at most twice as far as the fp32 torch
    loop's, labels equal where the float64 top-two gap exceeds 1e-5), the ATen form to those labels (its distance is printed)."""
    case = 6
    shape, roi, nc = tr.CASES[case]

    def run():
        net = tr.PredictorNet(nc, dev)
        out = val_3D.test_single_case_base(net, "unet_3D", wr.volume(shape).numpy(), 3, 3, roi, num_classes=nc, return_score=True,
                                           mode="gaussian", mirror_axes=(0, 1, 2))
        assert net.seen == 8 * len(wr.plan(shape, roi)[2])
        return out
    got, aten = _both_ways(monkeypatch, run)
    tr.softmax_bound(torch.from_numpy(got[1]), torch.from_numpy(got[0]), case, (0, 1, 2), 4, True, "kernel form")
    ref = tr.torch_loop(case, (0, 1, 2), 4, True, True, torch.float64)
    clear, _ = tr.clear_maxima(ref)
    print(f"|ATen form - fp64| {(torch.from_numpy(aten[1]).double() - ref['quot']).abs().max().item():.3e}")
    assert np.array_equal(aten[0][clear.numpy()], ref["label"].numpy()[clear.numpy()])


def test_all_case_base_scores_the_augmented_label_map(dev):
    """The metrics are those of the label map that the kernels give in the soft-max form (``kernel_loop``: the same launches)."""
    case, axes = 0, (0, 1)
    shape, roi, nc = tr.CASES[case]
    gt = synthetic_labels(shape, 7, nc).numpy().astype(np.uint8)
    got = val_3D.test_all_case_base(tr.PredictorNet(nc, dev), "unet_3D", None, num_classes=nc, patch_size=roi, stride_xy=6, stride_z=6,
                                    cases=[(wr.volume(shape).numpy(), gt)], mirror_axes=axes)
    label = tr.kernel_loop(case, axes, 4, True, False, dev)["label"].numpy()
    assert got == [[val_3D.cal_metric(gt == c, label == c)] for c in range(1, nc)]
    plain = tr.kernel_loop(case, None, 4, True, False, dev)["label"].numpy()
    assert (label != plain).any()      # the augmentation is visible in the label map that is scored


def test_all_case_amos_scores_the_augmented_label_map(dev):
    shape, nc = tr.AMOS_SHAPE, tr.AMOS_CLASSES
    gt = synthetic_labels((1, 1) + shape, 9, nc)
    net = tr.PredictorNet(nc, dev)
    got = val_3D.test_all_case_amos(net, "unet_3D", [{"image": wr.volume(shape)[None, None], "label": gt}], num_classes=nc,
                                    mirror_axes=tr.AMOS_AXES)
    assert net.seen == 8
    label, gt = tr.amos_label().numpy()[None], gt[0].numpy()
    assert got == [[val_3D.cal_metric(gt == c, label == c)] for c in range(1, nc)]


# ---- 6. a mirror-equivariant predictor ----

@pytest.mark.parametrize("case", CASE_PARAMS)
def test_pointwise_predictor_gains_nothing(dev, case):
    tr.check_equivariant(case, dev)


# ---- 7. refusals ----

def test_bad_masks_launch_nothing(dev):
    from icl_amd import _lib
    L = _lib.lib()
    roi, psize = (4, 4, 4), (8, 8, 8)
    vol = torch.ones((1, *psize), device=dev)
    out = torch.full((2, 1, *roi), 7.0, device=dev)
    score = torch.full((2, *psize), 7.0, device=dev)
    weight = torch.full(psize, 7.0, device=dev)
    logits = torch.ones((2, 2) + roi, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    origins = (ctypes.c_int32 * 6)(0, 0, 0, 4, 4, 4)
    for bad in (8, -1):
        flips = (ctypes.c_int32 * 2)(0, bad)
        calls = ((lambda: L.icl_window_gather_flipped(p(vol), p(out), origins, flips, 2, 1, *psize, 0, 0, 0, *psize, *roi, None), "window_gather_flipped"),
                 (lambda: L.icl_window_accumulate_flipped(p(logits), None, p(score), p(weight), origins, flips, 2, 2, *psize, *roi, 0, None),
                  "window_accumulate_flipped"))
        for call, who in calls:
            rc = call()
            msg = L.icl_last_error().decode()
            assert rc == -1 and who in msg and f"mask {bad}" in msg and "window 1" in msg, msg
    torch.cuda.synchronize()
    assert (out == 7).all() and (score == 7).all() and (weight == 7).all()
    for flips in ([0], [0, 1, 2], [0, 8]):
        with pytest.raises(ValueError, match="mirror mask"):
            ops.window_gather(vol, [(0, 0, 0), (4, 4, 4)], roi, (0, 0, 0), psize, flips=flips)
        with pytest.raises(ValueError, match="mirror mask"):
            ops.window_accumulate(logits, [(0, 0, 0), (4, 4, 4)], score, weight, flips=flips)
    for bad in ((0, 0), (3,), "x"):
        with pytest.raises(ValueError, match="mirror_axes"):
            val_3D.sliding_window_inference(vol[None], roi, 1, lambda w: w, mirror_axes=bad)
    assert (score == 7).all() and (weight == 7).all()
