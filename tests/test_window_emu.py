"""CPU checks of the sliding-window kernels (icl_amd/csrc/kernels/window.h) through tests/hipemu and the C ABI, and of the host side of
``icl_amd.val_3D`` that drives them.  Inputs, references and the assertions themselves are in tests/window_ref.py, shared with the GPU
tests:

  logits form     score map, weight map, quotients and label map EQUAL the fp32 torch loop's, with and without the importance map
  soft-max form   quotients at most twice as far from the float64 evaluation as the fp32 torch loop is; labels equal the float64
                  arg-max wherever its top-two gap exceeds 1e-5 (at most 1e-3 of the voxels may be left out)
"""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hipemu"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from build_emu import build_emu  # noqa: E402

import window_ref as wr  # noqa: E402
from icl_amd import _lib, ops, val_3D  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def emu_library():
    _lib._use_library_for_tests(build_emu(), host_pointers=True)
    yield
    _lib._use_library_for_tests(None)


CASE_PARAMS = [pytest.param(i, id=wr.IDS[i]) for i in range(len(wr.CASES))]


@pytest.mark.parametrize("gaussian", [False, True], ids=["constant", "gaussian"])
@pytest.mark.parametrize("sw_batch", [4, 1])
@pytest.mark.parametrize("case", CASE_PARAMS)
def test_logits_form_equals_the_fp32_torch_loop(case, sw_batch, gaussian):
    wr.check_logits_form(case, sw_batch, gaussian, "cpu")


@pytest.mark.parametrize("gaussian", [False, True], ids=["constant", "gaussian"])
@pytest.mark.parametrize("sw_batch", [4, 1])
@pytest.mark.parametrize("case", CASE_PARAMS)
def test_softmax_form_against_float64(case, sw_batch, gaussian):
    wr.check_softmax_form(case, sw_batch, gaussian, "cpu")


def test_gather_two_channels():
    wr.check_gather_two_channels("cpu")


def test_ties_and_nan():
    wr.check_ties("cpu")


def test_all_twelve_windows_in_one_launch():
    """One batch holds the whole grid of the second case: up to eight overlapping windows add to a voxel inside ONE launch."""
    case = 1
    wr.check_logits_form(case, 16, True, "cpu")


def _origins(*triples):
    flat = [v for t in triples for v in t]
    return (ctypes.c_int32 * len(flat))(*flat)


def test_bad_arguments_launch_nothing():
    L = _lib.lib()
    roi, psize = (4, 4, 4), (8, 8, 8)
    vol = torch.ones((1, *psize))
    out = torch.full((17, 1, *roi), 7.0)
    score = torch.full((257, *psize), 7.0)
    weight = torch.full(psize, 7.0)
    label = torch.full(psize, 7, dtype=torch.int64)
    logits = torch.ones((17, 257) + roi)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    good = _origins((0, 0, 0))

    def refused(rc, *words):
        assert rc == -1
        msg = L.icl_last_error().decode()
        assert all(w in msg for w in words), msg

    # 17 windows
    many = _origins(*[(0, 0, 0)] * 17)
    refused(L.icl_window_gather(p(vol), p(out), many, 17, 1, *psize, 0, 0, 0, *psize, *roi, None), "window_gather", "17 windows")
    refused(L.icl_window_accumulate(p(logits), None, p(score), p(weight), many, 17, 2, *psize, *roi, 0, None), "window_accumulate", "17 windows")
    # 257 classes (and none)
    refused(L.icl_window_accumulate(p(logits), None, p(score), p(weight), good, 1, 257, *psize, *roi, 0, None), "window_accumulate", "257 classes")
    refused(L.icl_window_accumulate(p(logits), None, p(score), p(weight), good, 1, 0, *psize, *roi, 0, None), "window_accumulate", "0 classes")
    refused(L.icl_window_finalize(p(score), p(weight), p(label), None, 257, *psize, 0, 0, 0, *psize, None), "window_finalize", "257 classes")
    # an origin that puts the window outside the padded extent, on either side
    for bad in ((0, 5, 0), (0, 0, -1)):
        o = _origins((0, 0, 0), bad)
        refused(L.icl_window_gather(p(vol), p(out), o, 2, 1, *psize, 0, 0, 0, *psize, *roi, None), "window_gather", "window 1", "outside")
        refused(L.icl_window_accumulate(p(logits), None, p(score), p(weight), o, 2, 2, *psize, *roi, 1, None), "window_accumulate", "outside")
    # a volume that does not fit the padded frame at its offset
    refused(L.icl_window_gather(p(vol), p(out), good, 1, 1, *psize, 1, 0, 0, *psize, *roi, None), "window_gather", "bad extents")
    refused(L.icl_window_finalize(p(score), p(weight), p(label), None, 2, *psize, 0, 0, 1, *psize, None), "window_finalize", "bad extents")
    # nothing was written
    assert (out == 7).all() and (score == 7).all() and (weight == 7).all() and (label == 7).all()
    with pytest.raises(RuntimeError, match="17 windows"):
        ops.window_gather(vol, [(0, 0, 0)] * 17, roi, (0, 0, 0), psize)


# ---- host side ------------------------------------------------------------------------------------------------------------------------

def _host_predictor(nc):
    return wr.CountingPredictor(nc)


@pytest.mark.parametrize("case", [0, 2], ids=[wr.IDS[0], wr.IDS[2]])
def test_sliding_window_inference_gaussian_equals_the_helper(case):
    """Host tensors take the ATen form, which offers the mode too; the kernel form of the same engine (``_run_windows``, here on the
    emulator) returns the same tensor."""
    shape, roi, nc = wr.CASES[case]
    want = wr.torch_loop(case, 4, False, True, torch.float32)["quot"]
    x = wr.volume(shape).reshape(1, 1, *shape)
    got = val_3D.sliding_window_inference(x, roi, 4, _host_predictor(nc), mode="gaussian")
    assert torch.equal(got[0], want)
    pads, psize, starts = wr.plan(shape, roi)
    (_, dev), handed = val_3D._run_windows(x, list(roi), pads, psize, [(0, *s) for s in starts], 4, _host_predictor(nc),
                                           wr.gaussian_map(roi), False, "quotients", True, val_3D._fits_amos(list(roi), x.device))
    assert handed is None and torch.equal(dev[0], want)
    plain = val_3D.sliding_window_inference(x, roi, 4, _host_predictor(nc))
    assert torch.equal(plain[0], wr.torch_loop(case, 4, False, False, torch.float32)["quot"])


def test_kernel_loop_over_a_batch_of_two_volumes():
    """Windows of two volumes share a forward (3 windows each, 4 per forward): the runs of one volume go to separate launches."""
    shape, roi, nc = (9, 4, 8), (4, 4, 8), 3
    x = torch.stack([wr.volume(shape), wr.volume(shape).flip(0)]).unsqueeze(1)
    want = val_3D.sliding_window_inference(x, roi, 4, _host_predictor(nc), mode="gaussian")
    pads = [(0, 0)] * 3
    starts = [(b, z, 0, 0) for b in range(2) for z in val_3D._scan_starts(9, 4, 0.25)]
    (_, got), handed = val_3D._run_windows(x, list(roi), pads, list(shape), starts, 4, _host_predictor(nc), wr.gaussian_map(roi), False,
                                           "quotients", True, val_3D._fits_amos(list(roi), x.device))
    assert handed is None and torch.equal(got, want)


def test_predictor_with_another_output_extent_falls_back():
    """The kernel loop hands its first prediction over instead of accumulating it (``ops.window_accumulate`` would refuse its shape with
    a ValueError), and the predictor is not asked for it again: the ATen form goes on with it and fails as it always has for a
    prediction that is not of the window's extent, in the broadcast of its first add (a RuntimeError)."""
    shape, roi = (6, 4, 8), (4, 4, 8)
    x = wr.volume(shape).reshape(1, 1, *shape)
    pads = [(0, 0)] * 3
    starts = [(0, z, 0, 0) for z in val_3D._scan_starts(6, 4, 0.25)]
    calls, handed = [], []

    def half(win):
        calls.append(win.shape[0])
        handed.append(win[..., ::2])
        return handed[-1]
    with pytest.raises(RuntimeError):
        val_3D._run_windows(x, list(roi), pads, list(shape), starts, 4, half, None, False, "quotients", True, val_3D._fits_amos(list(roi), x.device))
    assert tuple(handed[0].shape) == (len(starts), 1, 4, 4, 4) and calls == [len(starts)]


# the soft-max (BraTS) form of the engine's kernel loop, which host tensors never reach through ``test_single_case_base``

class _ScaleNet(torch.nn.Module):
    """x * w with w [1, C, 1, 1, 1], optionally cast or given one channel too many; counts its forwards."""

    def __init__(self, w, half=False, extra=False):
        super().__init__()
        self.w = torch.nn.Parameter(torch.tensor(w).view(1, -1, 1, 1, 1), requires_grad=False)
        self.half, self.extra, self.calls = half, extra, 0

    def forward(self, x):
        self.calls += 1
        y = x * self.w
        if self.extra:
            y = torch.cat([y, y[:, :1]], dim=1)
        return y.half() if self.half else y


def _brats_engine(net, shape, roi, nc, starts, per_forward, gaussian, want, kernels):
    """``_run_windows`` as ``_single_case_on_device`` calls it, on the host volume of ``window_ref``."""
    pads, psize, _ = wr.plan(shape, roi)
    imp = wr.gaussian_map(roi) if gaussian else None
    return val_3D._run_windows(wr.volume(shape)[None, None], roi, pads, psize, starts, per_forward, net, imp, True, want, kernels,
                               val_3D._fits_brats(nc, roi), nc)


@pytest.mark.parametrize("gaussian", [False, True], ids=["constant", "gaussian"])
def test_softmax_engine_seventeen_windows_in_one_forward(gaussian):
    """Volume (20, 4, 8), window (4, 4, 8) at stride 1 along the first axis: 17 windows in ONE forward, so the kernel loop splits the
    batch into launches of 16 + 1.  Against the ATen form of the same call: the score within 2e-6 (averages of probabilities <= 1 whose
    exponentials and sums may differ by a few ulp of 2^-23 between the two soft-maxes: the band of tests/test_gpu_window.py), the labels
    equal wherever the ATen score's top-two gap exceeds 1e-5 — which may leave out at most 1e-3 of the voxels (a condition on the inputs,
    checked on the ATen form alone first)."""
    shape, roi, nc = (20, 4, 8), (4, 4, 8), 3
    starts = [(0, x, 0, 0) for x in range(17)]
    w = [0.5, -1.0, 2.0]
    (lab_a, score_a), _ = _brats_engine(_ScaleNet(w), shape, roi, nc, starts, 17, gaussian, "both", False)
    top = torch.topk(score_a[0], 2, dim=0).values
    clear = (top[0] - top[1]) > 1e-5
    left_out = 1.0 - clear.double().mean().item()
    print(f"voxels with a top-two gap <= 1e-5 in the ATen score: {left_out:.3e}")
    assert left_out <= 1e-3, left_out
    net = _ScaleNet(w)
    (lab_k, score_k), handed = _brats_engine(net, shape, roi, nc, starts, 17, gaussian, "both", True)
    assert handed is None and net.calls == 1
    assert lab_k.shape == lab_a.shape == (1, *shape) and lab_k.dtype == torch.int64 and score_k.shape == score_a.shape == (1, nc, *shape)
    print(f"score: largest difference {(score_k - score_a).abs().max().item():.3e}; labels that differ: {(lab_k != lab_a).float().mean().item():.3e}")
    assert (score_k - score_a).abs().max().item() <= 2e-6
    assert torch.equal(lab_k[0][clear], lab_a[0][clear])


@pytest.mark.parametrize("why", ["fp16", "one channel too many"])
def test_softmax_engine_hands_its_first_batch_over(why):
    """A network whose output is fp16, or has num_classes + 1 channels, leaves the kernel loop at its first batch: that prediction is
    handed over, and the network is called as often as by the ATen form."""
    shape, roi, nc = (9, 4, 8), (4, 4, 8), 3
    starts = [(0, x, 0, 0) for x in (0, 3, 5)]
    w = [0.5, -1.0, 2.0]
    kw = {"half": True} if why == "fp16" else {"extra": True}
    net_k, net_a = _ScaleNet(w, **kw), _ScaleNet(w, **kw)
    if why != "fp16":      # four channels do not go into a three-class score map: the ATen form refuses them at its first add, as it always has
        for net, kernels in ((net_k, True), (net_a, False)):
            with pytest.raises(RuntimeError):
                _brats_engine(net, shape, roi, nc, starts, 2, False, "both", kernels)
        assert net_k.calls == net_a.calls == 1
        return
    (lab_k, score_k), handed = _brats_engine(net_k, shape, roi, nc, starts, 2, False, "both", True)
    (lab_a, score_a), none = _brats_engine(net_a, shape, roi, nc, starts, 2, False, "both", False)
    assert tuple(handed.shape) == (2, nc, *roi) and handed.dtype == torch.float16 and none is None
    assert net_k.calls == net_a.calls == 2
    assert torch.equal(lab_k, lab_a) and torch.equal(score_k, score_a)


def test_softmax_engine_padded_and_cropped():
    """Volume (5, 12, 6) under a window of (8, 12, 8), the third case of ``window_ref``: the gather zero-fills, the finalize crops.  The
    label-only call returns the label map of the label-and-score call, and both forms of the engine agree with the independent fp32
    loop of ``window_ref.torch_loop`` — the ATen form exactly, the kernel form within the 2e-6 band of the soft-max, with equal labels
    wherever that loop's top-two gap exceeds 1e-5."""
    case = 2
    shape, roi, nc = wr.CASES[case]
    starts = [(0, *s) for s in wr.plan(shape, roi)[2]]
    want = wr.torch_loop(case, 4, True, True, torch.float32)
    (lab_both, score), _ = _brats_engine(wr.CountingPredictor(nc), shape, roi, nc, starts, 4, True, "both", True)
    (lab_only, none), _ = _brats_engine(wr.CountingPredictor(nc), shape, roi, nc, starts, 4, True, "label", True)
    assert none is None and lab_only.shape == (1, *shape) and score.shape == (1, nc, *shape)
    assert torch.equal(lab_only, lab_both)
    (lab_a, score_a), _ = _brats_engine(wr.CountingPredictor(nc), shape, roi, nc, starts, 4, True, "both", False)
    assert torch.equal(score_a[0], want["quot"]) and torch.equal(lab_a[0], want["label"])
    top = torch.topk(want["quot"], 2, dim=0).values
    clear = (top[0] - top[1]) > 1e-5
    assert 1.0 - clear.double().mean().item() <= 1e-3
    print(f"score: largest difference from window_ref's fp32 loop {(score[0] - want['quot']).abs().max().item():.3e}")
    assert (score[0] - want["quot"]).abs().max().item() <= 2e-6
    assert torch.equal(lab_both[0][clear], want["label"][clear])


def test_unknown_mode_raises():
    x = torch.zeros((1, 1, 4, 4, 4))
    with pytest.raises(ValueError, match="mode"):
        val_3D.sliding_window_inference(x, (4, 4, 4), 1, lambda w: w, mode="linear")
    net = torch.nn.Conv3d(1, 2, 1)
    with pytest.raises(ValueError, match="mode"):
        val_3D.test_single_case_base(net, "unet_3D", x[0, 0].numpy(), 2, 2, (4, 4, 4), num_classes=2, mode="linear")


def test_single_case_gaussian_on_the_host():
    """``test_single_case_base(mode="gaussian")`` on a CPU net (ATen loop) against the weighted average written out here."""
    torch.manual_seed(0)
    net = torch.nn.Conv3d(1, 3, 1)
    image = wr.volume((9, 4, 8)).numpy()
    label, score = val_3D.test_single_case_base(net, "unet_3D", image, 3, 3, (4, 4, 8), num_classes=3, return_score=True, mode="gaussian")
    imp = wr.gaussian_map((4, 4, 8))
    acc, wsum = torch.zeros((3, 9, 4, 8)), torch.zeros((9, 4, 8))
    with torch.no_grad():
        for z in (0, 3, 5):
            prob = torch.softmax(net(torch.from_numpy(image[None, None, z:z + 4])), dim=1)[0]
            acc[:, z:z + 4] += prob * imp
            wsum[z:z + 4] += imp
    assert torch.equal(torch.from_numpy(score), acc / wsum)
    assert torch.equal(torch.from_numpy(label), torch.argmax(acc / wsum, dim=0))


def test_val_windows_switch(monkeypatch):
    monkeypatch.delenv("ICL_VAL_WINDOWS", raising=False)
    assert val_3D.val_windows_mode() == "device"
    for way in ("device", "aten"):
        monkeypatch.setenv("ICL_VAL_WINDOWS", way)
        assert val_3D.val_windows_mode() == way
    monkeypatch.setenv("ICL_VAL_WINDOWS", "bogus")
    with pytest.raises(ValueError, match="ICL_VAL_WINDOWS"):
        val_3D.val_windows_mode()


@pytest.mark.parametrize("roi", [(7, 5, 9), (8, 12, 8), (96, 96, 96)])
def test_gaussian_map(roi):
    m = val_3D.gaussian_importance_map(roi)
    assert m.dtype == torch.float32 and tuple(m.shape) == roi
    c = tuple(r // 2 for r in roi)
    assert m[c] == 1.0 and m.max() == 1.0
    assert m.min() >= 1e-3
    assert torch.equal(m, wr.gaussian_map(roi))
    for ax, r in enumerate(roi):
        if r % 2:      # odd extent: symmetric about the centre
            assert torch.equal(m, m.flip(ax))
    if roi == (96, 96, 96):
        assert m[0, 0, 0] == 1e-3      # the floor is reached in the corners
