"""GPU tests of the sliding-window kernels (run with -m gpu; icl_amd/csrc/kernels/window.h) and of the two validation loops of
``icl_amd.val_3D`` on top of them.

The kernel cases, their references and their assertions are those of tests/test_window_emu.py (tests/window_ref.py): equality with the
fp32 torch loop in the logits form, the float64 bounds in the soft-max form.  The loops are compared with their ATen form behind
``ICL_VAL_WINDOWS=aten`` on a hash-filled HIP ``unet_3D``: equal logits for the AMOS loop (it adds logits: the same adds in the same
order), Dice within 1e-4 and HD95 within 1.0 for the BraTS loop (only the soft-max's last bits differ; the bands of
tests/test_gpu_dropin.py for a reordered evaluation of one network).
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import window_ref as wr  # noqa: E402
from icl_amd import val_3D  # noqa: E402
from icl_amd.utils.hashfill import fill_like_reference_init, synthetic_labels, synthetic_volume  # noqa: E402

pytestmark = pytest.mark.gpu

CASE_PARAMS = [pytest.param(i, id=wr.IDS[i]) for i in range(len(wr.CASES))]


@pytest.fixture(scope="module")
def dev():
    from icl_amd import _lib
    assert _lib.lib_path().endswith("libicl_hip.so"), "GPU tests must run on the HIP library"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def net(dev):
    from icl_amd.networks.unet_3D import unet_3D
    model = unet_3D(n_classes=3, in_channels=1, device=dev)
    fill_like_reference_init(list(model.named_parameters()))
    return model.eval()


@pytest.mark.parametrize("gaussian", [False, True], ids=["constant", "gaussian"])
@pytest.mark.parametrize("sw_batch", [4, 1])
@pytest.mark.parametrize("case", CASE_PARAMS)
def test_logits_form_equals_the_fp32_torch_loop(dev, case, sw_batch, gaussian):
    wr.check_logits_form(case, sw_batch, gaussian, dev)


@pytest.mark.parametrize("gaussian", [False, True], ids=["constant", "gaussian"])
@pytest.mark.parametrize("sw_batch", [4, 1])
@pytest.mark.parametrize("case", CASE_PARAMS)
def test_softmax_form_against_float64(dev, case, sw_batch, gaussian):
    wr.check_softmax_form(case, sw_batch, gaussian, dev)


def test_gather_two_channels(dev):
    wr.check_gather_two_channels(dev)


def test_ties_and_nan(dev):
    wr.check_ties(dev)


def _both_ways(monkeypatch, fn):
    out = {}
    for way in ("device", "aten"):
        monkeypatch.setenv("ICL_VAL_WINDOWS", way)
        out[way] = fn()
    return out["device"], out["aten"]


@pytest.mark.parametrize("mode", ["constant", "gaussian"])
def test_sliding_window_inference_equals_the_aten_loop(dev, net, monkeypatch, mode):
    """2 x 1 x 2 windows of 32^3 over (40, 32, 45), one forward of four; last-axis origins 0 and 13."""
    x = synthetic_volume((1, 1, 40, 32, 45), 11).to(dev)
    got, want = _both_ways(monkeypatch, lambda: val_3D.sliding_window_inference(x, (32, 32, 32), 4, net, mode=mode))
    assert got.shape == want.shape == (1, 3, 40, 32, 45) and got.dtype == torch.float32
    assert torch.equal(got, want)
    assert torch.isfinite(got).all() and got.std() > 0


def test_amos_loop_equals_the_aten_loop(dev, net, monkeypatch):
    """`test_all_case_amos` (96^3 windows: the volume is zero-padded on every axis by the gather and cropped by the finalize)."""
    shape = (40, 32, 45)
    loader = [{"image": synthetic_volume((1, 1) + shape, 11), "label": synthetic_labels((1, 1) + shape, 12, 3)}]
    got, want = _both_ways(monkeypatch, lambda: val_3D.test_all_case_amos(net, "unet_3D", loader, num_classes=3))
    assert len(got) == 2 and all(len(m) == 1 for m in got)
    assert got == want


def test_brats_loop_within_the_bands_of_the_aten_loop(dev, net, monkeypatch):
    """`test_all_case_base` on two cases; the second one is narrower than the window on its first axis (padding)."""
    cases = [(synthetic_volume(s, 21 + i).numpy(), synthetic_labels(s, 31 + i, 3).numpy().astype(np.uint8))
             for i, s in enumerate([(40, 32, 45), (30, 36, 32)])]
    got, want = _both_ways(monkeypatch, lambda: val_3D.test_all_case_base(net, "unet_3D", None, num_classes=3, patch_size=(32, 32, 32),
                                                                          stride_xy=16, stride_z=16, cases=cases))
    assert len(got) == len(want) == 2
    for c, (g_cls, w_cls) in enumerate(zip(got, want), 1):
        assert len(g_cls) == len(w_cls) == 2
        for g, w in zip(g_cls, w_cls):
            print(f"class {c}: device {g}, aten {w}")
            assert abs(g[0] - w[0]) <= 1e-4 and abs(g[1] - w[1]) <= 1.0, (c, g, w)
    # the label map and the score of one case, both ways: the maps differ at arg-max near-ties only
    monkeypatch.setenv("ICL_VAL_WINDOWS", "device")
    lab_d, score_d = val_3D.test_single_case_base(net, "unet_3D", cases[1][0], 16, 16, (32, 32, 32), num_classes=3, return_score=True)
    monkeypatch.setenv("ICL_VAL_WINDOWS", "aten")
    lab_a, score_a = val_3D.test_single_case_base(net, "unet_3D", cases[1][0], 16, 16, (32, 32, 32), num_classes=3, return_score=True)
    assert lab_d.shape == lab_a.shape == (30, 36, 32) and lab_d.dtype == lab_a.dtype
    assert score_d.shape == score_a.shape == (3, 30, 36, 32)
    print(f"score: largest difference {np.abs(score_d - score_a).max():.3e}; labels that differ: {(lab_d != lab_a).mean():.3e}")
    # averages of probabilities (<= 1) whose exponentials and sums may differ by a few ulp (2^-23 each) between the two soft-maxes
    assert np.abs(score_d - score_a).max() <= 2e-6


def test_device_path_allocates_less(dev, monkeypatch):
    """One AMOS-style call at 8 classes on 64^3 with 32^3 windows (27 windows, 7 forwards) and a predictor that allocates nothing: the
    kernel path needs no padded copy, no per-window temporaries and no second class-by-volume tensor for the quotients."""
    x = synthetic_volume((1, 1, 64, 64, 64), 3).to(dev)
    logits = synthetic_volume((4, 8, 32, 32, 32), 4).to(dev)
    peaks, outs = {}, {}
    for way in ("device", "aten"):
        monkeypatch.setenv("ICL_VAL_WINDOWS", way)
        torch.cuda.synchronize()
        start = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        outs[way] = val_3D.sliding_window_inference(x, (32, 32, 32), 4, lambda win: logits[:win.shape[0]])
        torch.cuda.synchronize()
        peaks[way] = torch.cuda.max_memory_allocated() - start
    print(f"peak bytes above the start: device {peaks['device']}, aten {peaks['aten']}")
    assert torch.equal(outs["device"], outs["aten"])
    assert peaks["device"] < peaks["aten"], peaks


def test_fallback_sees_every_batch_once(dev, monkeypatch):
    """A network whose output is not fp32 leaves the kernel loop at its first batch; the ATen loop takes that batch over, so the result
    and the number of forwards are those of ``ICL_VAL_WINDOWS=aten``."""
    class HalfNet(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.tensor([0.5, -1.0, 2.0], device=dev).view(1, 3, 1, 1, 1), requires_grad=False)
            self.calls = 0

        def forward(self, x):
            self.calls += 1
            return (x * self.w).half()
    image = synthetic_volume((20, 16, 21), 41).numpy()
    out, calls = {}, {}
    for way in ("device", "aten"):
        monkeypatch.setenv("ICL_VAL_WINDOWS", way)
        net = HalfNet()
        out[way] = val_3D.test_single_case_base(net, "unet_3D", image, 8, 8, (16, 16, 16), num_classes=3, return_score=True)
        calls[way] = net.calls
    assert calls["device"] == calls["aten"] == 1      # 2 x 1 x 2 windows, four per forward
    assert np.array_equal(out["device"][0], out["aten"][0]) and np.array_equal(out["device"][1], out["aten"][1])


@pytest.mark.parametrize("mode", ["constant", "gaussian"])
def test_brats_loop_seventeen_windows_in_one_forward(dev, monkeypatch, mode):
    """Volume (20, 4, 8), window (4, 4, 8) at stride 1: the 17 windows of the grid go through ONE forward, which the kernel loop splits into
    launches of 16 + 1.  Against ``ICL_VAL_WINDOWS=aten``: the score within 2e-6 (the band of the BraTS test above, for the same
    reason), the labels equal wherever the ATen score's top-two gap exceeds 1e-5, which leaves out at most 1e-3 of the voxels."""
    class ScaleNet(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.tensor([0.5, -1.0, 2.0], device=dev).view(1, 3, 1, 1, 1), requires_grad=False)
            self.calls = 0

        def forward(self, x):
            self.calls += 1
            return x * self.w
    image = wr.volume((20, 4, 8)).numpy()
    out = {}
    for way in ("device", "aten"):
        monkeypatch.setenv("ICL_VAL_WINDOWS", way)
        net = ScaleNet()
        out[way] = val_3D.test_single_case_base(net, "unet_3D", image, 1, 1, (4, 4, 8), num_classes=3, windows_per_batch=17, return_score=True,
                                                mode=mode)
        assert net.calls == 1
    (lab_d, score_d), (lab_a, score_a) = out["device"], out["aten"]
    assert lab_d.shape == lab_a.shape == (20, 4, 8) and lab_d.dtype == lab_a.dtype and score_d.shape == score_a.shape == (3, 20, 4, 8)
    top = np.sort(score_a, axis=0)
    clear = (top[-1] - top[-2]) > 1e-5
    print(f"score: largest difference {np.abs(score_d - score_a).max():.3e}; labels that differ: {(lab_d != lab_a).mean():.3e}; "
          f"voxels with a top-two gap <= 1e-5: {1.0 - clear.mean():.3e}")
    assert 1.0 - clear.mean() <= 1e-3
    assert np.abs(score_d - score_a).max() <= 2e-6
    assert np.array_equal(lab_d[clear], lab_a[clear])
