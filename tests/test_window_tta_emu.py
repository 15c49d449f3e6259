"""CPU checks of mirror test-time augmentation in the sliding-window kernels (icl_amd/csrc/kernels/window.h: the WinFlips instantiations of
``window_gather_kernel`` and ``window_accumulate_kernel``) through tests/hipemu and the C ABI, and of ``mirror_axes=`` in
``icl_amd.val_3D``.  The definition, the reference loop and the assertions are in tests/window_tta_ref.py, shared with the GPU tests
(tests/test_gpu_window_tta.py).  Host tensors take the ATen form in ``val_3D``; its kernel form is reached here through ``_run_windows``
on the emulator.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hipemu"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from build_emu import build_emu  # noqa: E402

import window_ref as wr  # noqa: E402
import window_tta_ref as tr  # noqa: E402
from icl_amd import _lib, ops, val_3D  # noqa: E402
from icl_amd.utils.hashfill import synthetic_labels  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def emu_library():
    _lib._use_library_for_tests(build_emu(), host_pointers=True)
    yield
    _lib._use_library_for_tests(None)


CASE_PARAMS = [pytest.param(i, id=tr.IDS[i]) for i in range(len(tr.CASES))]
AXES_PARAMS = [pytest.param(a, id="axes" + "".join(map(str, a))) for a in tr.MIRROR_AXES]
SOFTMAX_PARAMS = [pytest.param(i, a, id=f"{tr.IDS[i]}-axes{''.join(map(str, a))}") for i in range(len(tr.CASES)) for a in tr.MIRROR_AXES
                  if (i, a) not in tr.SOFTMAX_LEFT_OUT]


# ---- 1. gather ----

@pytest.mark.parametrize("case", CASE_PARAMS)
def test_gather_equals_torch_flip(case):
    tr.check_gather(case, "cpu")


def test_gather_two_channels():
    tr.check_gather_two_channels("cpu")


# ---- 2. logits form ----

@pytest.mark.parametrize("gaussian", [False, True], ids=["constant", "gaussian"])
@pytest.mark.parametrize("per_forward", [1, 4, 16])
@pytest.mark.parametrize("axes", AXES_PARAMS)
@pytest.mark.parametrize("case", CASE_PARAMS)
def test_logits_form_equals_the_fp32_torch_loop(case, axes, per_forward, gaussian):
    tr.check_logits_form(case, axes, per_forward, gaussian, "cpu")


# ---- 3. soft-max form ----

@pytest.mark.parametrize("gaussian", [False, True], ids=["constant", "gaussian"])
@pytest.mark.parametrize("case", range(len(tr.CASES)), ids=tr.IDS)
@pytest.mark.parametrize("axes", AXES_PARAMS)
def test_softmax_inputs_have_clear_maxima(case, axes, gaussian):
    """The condition on the inputs of the soft-max checks (here and on the GPU), from the float64 torch loop alone: at most 1e-3 of the
    voxels have a top-two gap <= 1e-5 — for every (case, mirror_axes) that is not listed in ``SOFTMAX_LEFT_OUT``; the listed ones break it
    (that is why they are listed).  Every class layout (C <= 4, <= 16, > 16) keeps a case."""
    _, left_out = tr.clear_maxima(tr.torch_loop(case, axes, 4, True, gaussian, torch.float64))
    print(f"{tr.IDS[case]} axes {axes} gaussian {gaussian}: voxels with a float64 top-two gap <= 1e-5: {left_out:.3e}")
    if (case, axes) not in tr.SOFTMAX_LEFT_OUT:
        assert left_out <= 1e-3
    else:
        assert left_out > 1e-3      # listed for this reason and no other
    for lay in (lambda c: c <= 4, lambda c: 4 < c <= 16, lambda c: c > 16):
        assert any(lay(tr.CASES[i][2]) and (i, a) not in tr.SOFTMAX_LEFT_OUT for i in range(len(tr.CASES)) for a in tr.MIRROR_AXES)


@pytest.mark.parametrize("gaussian", [False, True], ids=["constant", "gaussian"])
@pytest.mark.parametrize("per_forward", [4, 16])
@pytest.mark.parametrize("case,axes", SOFTMAX_PARAMS)
def test_softmax_form_against_float64(case, axes, per_forward, gaussian):
    tr.check_softmax_form(case, axes, per_forward, gaussian, "cpu")


# ---- 4. / 5. the host loops: ``_run_windows`` in its kernel form on the emulator, the public functions in their ATen form ----

def _engine(case, per_forward, predictor, gaussian, softmax, want, kernels, mirror_axes, fits=None):
    shape, roi, nc = tr.CASES[case]
    pads, psize, starts = wr.plan(shape, roi)
    x = wr.volume(shape)[None, None]
    imp = wr.gaussian_map(roi) if gaussian else None
    fits = fits or (val_3D._fits_brats(nc, roi) if softmax else val_3D._fits_amos(list(roi), x.device))
    return val_3D._run_windows(x, list(roi), pads, psize, [(0, *s) for s in starts], per_forward, predictor, imp, softmax, want, kernels, fits,
                               nc if softmax else None, masks=val_3D._mirror_masks(mirror_axes))


@pytest.mark.parametrize("softmax", [False, True], ids=["logits", "softmax"])
@pytest.mark.parametrize("case", [0, 2], ids=[tr.IDS[0], tr.IDS[2]])
def test_empty_mirror_axes_is_no_augmentation(case, softmax):
    """``mirror_axes=()``: one pass per window with mask 0 — bit-equal to ``None``, on the kernel form (mask-0 launches of the WinFlips
    instantiations against the plain ones) and through the public functions."""
    shape, roi, nc = tr.CASES[case]
    (lab_n, quot_n), _ = _engine(case, 4, wr.CountingPredictor(nc), True, softmax, "both", True, None)
    (lab_e, quot_e), _ = _engine(case, 4, wr.CountingPredictor(nc), True, softmax, "both", True, ())
    assert torch.equal(lab_n, lab_e) and torch.equal(quot_n, quot_e)
    x = wr.volume(shape)[None, None]
    if softmax:
        image = wr.volume(shape).numpy()
        a = val_3D.test_single_case_base(tr.PredictorNet(nc), "unet_3D", image, 6, 6, roi, num_classes=nc, return_score=True)
        b = val_3D.test_single_case_base(tr.PredictorNet(nc), "unet_3D", image, 6, 6, roi, num_classes=nc, return_score=True, mirror_axes=())
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    else:
        a = val_3D.sliding_window_inference(x, roi, 4, wr.CountingPredictor(nc), mode="gaussian")
        b = val_3D.sliding_window_inference(x, roi, 4, wr.CountingPredictor(nc), mode="gaussian", mirror_axes=())
        assert torch.equal(a, b)


@pytest.mark.parametrize("gaussian", [False, True], ids=["constant", "gaussian"])
def test_sliding_window_inference_all_mirrors(gaussian):
    """``sliding_window_inference(mirror_axes=(0, 1, 2))``: the predictor sees 8 x windows samples; the result (ATen form: a host tensor)
    is the reference loop's, and the kernel form of the same engine returns the same tensor."""
    case = 0
    shape, roi, nc = tr.CASES[case]
    windows = len(wr.plan(shape, roi)[2])
    want = tr.torch_loop(case, (0, 1, 2), 4, False, gaussian, torch.float32)["quot"]
    pred = wr.CountingPredictor(nc)
    got = val_3D.sliding_window_inference(wr.volume(shape)[None, None], roi, 4, pred, mode="gaussian" if gaussian else "constant",
                                          mirror_axes=(0, 1, 2))
    assert pred.seen == 8 * windows and torch.equal(got[0], want)
    pred = wr.CountingPredictor(nc)
    (_, quot), handed = _engine(case, 4, pred, gaussian, False, "quotients", True, (0, 1, 2))
    assert handed is None and pred.seen == 8 * windows and torch.equal(quot[0], want)


def test_hand_over_in_the_middle_of_the_mirrors():
    """A first prediction that ``fits`` refuses leaves the kernel form after the first batch of PASSES (5 per forward: the batch ends
    inside a window's eight mirrors): that prediction is used once, every pass goes through the predictor once, and the result is the
    ATen form's.  Logits form: 257 classes are more than the kernels take; soft-max form: an fp16 prediction."""
    case = 0
    shape, roi, nc = tr.CASES[case]
    windows = len(wr.plan(shape, roi)[2])
    k, a = wr.CountingPredictor(257), wr.CountingPredictor(257)
    (_, quot_k), handed = _engine(case, 5, k, True, False, "quotients", True, (0, 1, 2))
    (_, quot_a), none = _engine(case, 5, a, True, False, "quotients", False, (0, 1, 2))
    assert tuple(handed.shape) == (5, 257, *roi) and none is None and k.seen == a.seen == 8 * windows
    assert torch.equal(quot_k, quot_a)
    k, a = tr.PredictorNet(nc, dtype=torch.float16), tr.PredictorNet(nc, dtype=torch.float16)
    (lab_k, quot_k), handed = _engine(case, 5, k, True, True, "both", True, (0, 1, 2))
    (lab_a, quot_a), none = _engine(case, 5, a, True, True, "both", False, (0, 1, 2))
    assert handed.dtype == torch.float16 and none is None and k.seen == a.seen == 8 * windows and k.calls == a.calls
    assert torch.equal(quot_k, quot_a) and torch.equal(lab_k, lab_a)


def test_single_case_base_all_mirrors():
    """``test_single_case_base(mirror_axes=(0, 1, 2))`` on an ``nn.Module`` around the synthetic predictor; on the last case (8 windows,
    9 classes) strides of 3 give the grid of ``window_ref.plan``.  The ATen form (a host module) equals the fp32 reference loop; the
    kernel form of the engine holds the soft-max bound against float64."""
    case = 6
    shape, roi, nc = tr.CASES[case]
    net = tr.PredictorNet(nc)
    label, score = val_3D.test_single_case_base(net, "unet_3D", wr.volume(shape).numpy(), 3, 3, roi, num_classes=nc, return_score=True,
                                                mode="gaussian", mirror_axes=(0, 1, 2))
    want = tr.torch_loop(case, (0, 1, 2), 4, True, True, torch.float32)
    assert net.seen == 8 * len(wr.plan(shape, roi)[2])
    assert torch.equal(torch.from_numpy(score), want["quot"]) and torch.equal(torch.from_numpy(label), want["label"])
    (lab_k, quot_k), _ = _engine(case, 4, tr.PredictorNet(nc), True, True, "both", True, (0, 1, 2))
    tr.softmax_bound(quot_k[0], lab_k[0], case, (0, 1, 2), 4, True, "kernel form")


def test_all_case_base_scores_the_augmented_label_map():
    case, axes = 0, (0, 1)
    shape, roi, nc = tr.CASES[case]
    gt = synthetic_labels(shape, 7, nc).numpy().astype(np.uint8)
    got = val_3D.test_all_case_base(tr.PredictorNet(nc), "unet_3D", None, num_classes=nc, patch_size=roi, stride_xy=6, stride_z=6,
                                    cases=[(wr.volume(shape).numpy(), gt)], mirror_axes=axes)
    label = tr.torch_loop(case, axes, 4, True, False, torch.float32)["label"].numpy()
    assert got == [[val_3D.cal_metric(gt == c, label == c)] for c in range(1, nc)]
    plain = tr.torch_loop(case, None, 4, True, False, torch.float32)["label"].numpy()
    assert (label != plain).any()      # the augmentation is visible in the label map that is scored


def test_all_case_amos_scores_the_augmented_label_map():
    shape, nc = tr.AMOS_SHAPE, tr.AMOS_CLASSES
    gt = synthetic_labels((1, 1) + shape, 9, nc)
    net = tr.PredictorNet(nc)
    got = val_3D.test_all_case_amos(net, "unet_3D", [{"image": wr.volume(shape)[None, None], "label": gt}], num_classes=nc,
                                    mirror_axes=tr.AMOS_AXES)
    assert net.seen == 8
    label, gt = tr.amos_label().numpy()[None], gt[0].numpy()
    assert got == [[val_3D.cal_metric(gt == c, label == c)] for c in range(1, nc)]


# ---- 6. a mirror-equivariant predictor ----

@pytest.mark.parametrize("case", CASE_PARAMS)
def test_pointwise_predictor_gains_nothing(case):
    tr.check_equivariant(case, "cpu")


# ---- 7. refusals ----

def test_bad_masks_launch_nothing():
    L = _lib.lib()
    roi, psize = (4, 4, 4), (8, 8, 8)
    vol = torch.ones((1, *psize))
    out = torch.full((2, 1, *roi), 7.0)
    score = torch.full((2, *psize), 7.0)
    weight = torch.full(psize, 7.0)
    logits = torch.ones((2, 2) + roi)
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
    # today's refusals hold for the new entry points too
    many, zeros = (ctypes.c_int32 * 51)(), (ctypes.c_int32 * 17)()
    assert L.icl_window_gather_flipped(p(vol), p(out), many, zeros, 17, 1, *psize, 0, 0, 0, *psize, *roi, None) == -1
    assert "window_gather_flipped" in L.icl_last_error().decode() and "17 windows" in L.icl_last_error().decode()
    assert L.icl_window_accumulate_flipped(p(logits), None, p(score), p(weight), origins, None, 2, 2, *psize, *roi, 0, None) == -1
    assert "null pointer" in L.icl_last_error().decode()
    assert (out == 7).all() and (score == 7).all() and (weight == 7).all()
    for flips in ([0], [0, 1, 2], [0, 8], [0, -1], [0, 1.0]):
        with pytest.raises(ValueError, match="mirror mask"):
            ops.window_gather(vol, [(0, 0, 0), (4, 4, 4)], roi, (0, 0, 0), psize, flips=flips)
        with pytest.raises(ValueError, match="mirror mask"):
            ops.window_accumulate(logits, [(0, 0, 0), (4, 4, 4)], score, weight, flips=flips)
    assert (score == 7).all() and (weight == 7).all()


@pytest.mark.parametrize("bad", [(0, 0), (3,), "x", (-1,), (1.0,), 2, (True,)])
def test_bad_mirror_axes_raise(bad):
    x = torch.zeros((1, 1, 4, 4, 4))
    net = torch.nn.Conv3d(1, 2, 1)
    with pytest.raises(ValueError, match="mirror_axes"):
        val_3D.sliding_window_inference(x, (4, 4, 4), 1, lambda w: w, mirror_axes=bad)
    with pytest.raises(ValueError, match="mirror_axes"):
        val_3D.test_single_case_base(net, "unet_3D", x[0, 0].numpy(), 2, 2, (4, 4, 4), num_classes=2, mirror_axes=bad)
    with pytest.raises(ValueError, match="mirror_axes"):
        val_3D.test_all_case_base(net, "unet_3D", None, num_classes=2, cases=[], mirror_axes=bad)
    with pytest.raises(ValueError, match="mirror_axes"):
        val_3D.test_all_case_amos(net, "unet_3D", [], num_classes=2, mirror_axes=bad)


def test_mirror_axes_need_a_3d_input():
    x = torch.zeros((1, 1, 4, 4))
    with pytest.raises(ValueError, match="3-D"):
        val_3D.sliding_window_inference(x, (4, 4), 1, lambda w: w, mirror_axes=())


def test_masks_come_in_increasing_order():
    assert val_3D._mirror_masks(None) is None and val_3D._mirror_masks(()) == [0]
    for axes in [(2,), (0, 1), (2, 0), (0, 1, 2), (2, 1, 0), [1]]:
        assert val_3D._mirror_masks(axes) == tr.masks_of(tuple(axes))
    assert val_3D._mirror_masks((2, 0)) == [0, 1, 4, 5]
