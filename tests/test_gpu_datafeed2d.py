"""2-D data feed and slice resize on the MI355X, through the C ABI (slice_augment_kernel / slice_resize_kernel in
csrc/kernels/datafeed.h): bit for bit the reference's scipy chain (goldens of tests/golden/make_golden_datafeed2d.py), and the 2-D
validation loop with the device resize equal to the one with scipy on the host."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from test_datafeed2d import (REAL, SMALL, check_mixed_batch, check_real_cases, check_resize_cases, check_small_cases,  # noqa: E402
                             device_real_case)

from icl_amd import val_2D  # noqa: E402
from icl_amd.utils.hashfill import fill_like_reference_init, synthetic_segmentation, synthetic_volume  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from icl_amd import _lib
    assert _lib.lib_path().endswith("libicl_hip.so"), "GPU tests must run on the HIP library"
    return torch.device("cuda", 0)


def test_fused_generator_kernel_equals_the_reference_on_the_gpu(dev):
    store = check_small_cases(dev)
    assert len(store) == len(SMALL) and store.images[0].is_cuda
    check_mixed_batch(store, 24, (64, 48), 79)          # the U-Net trainer's batch in one call
    check_mixed_batch(store, 40, (24, 20), 80)          # 32 samples, then 8


def test_fused_generator_kernel_at_the_real_extents(dev):
    assert len(REAL) == 30
    check_real_cases(device_real_case(dev))


def test_slice_resize_equals_scipy_zoom_on_the_gpu(dev):
    check_resize_cases(dev)


def _zero_edge_case(seed):
    """6 x 78 x 58 slices at patch 64 x 48: 58 -> 48 going in (a zero last column of the network's input) and 64 -> 78 coming back (a
    zero last row of the prediction) both hit scipy's zero-edge rule."""
    gt, _ = synthetic_segmentation((6, 78, 58), 4, seed)
    image = torch.from_numpy(synthetic_volume((6, 78, 58), seed + 1).numpy() + gt.astype(np.float32)).unsqueeze(0)
    return image, torch.from_numpy(gt).unsqueeze(0)


def _scipy_forbidden(*args, **kwargs):
    raise AssertionError("the device run resized a slice on the host")


def _resize_both_ways(monkeypatch, fn):
    """fn() under ICL_VAL_RESIZE=host, then under =device with val_2D's scipy zoom made to fail if called."""
    monkeypatch.setenv("ICL_VAL_RESIZE", "host")
    want = fn()
    monkeypatch.setenv("ICL_VAL_RESIZE", "device")
    with monkeypatch.context() as m:
        m.setattr(val_2D, "zoom", _scipy_forbidden)
        got = fn()
    return got, want


@pytest.mark.parametrize("entry", ["test_single_volume_ours", "test_single_volume"])
def test_2d_validation_device_resize_equals_host_resize(dev, monkeypatch, entry):
    from icl_amd.networks.net_factory import net_factory
    ours = entry == "test_single_volume_ours"
    model = net_factory(net_type="icl_unet" if ours else "unet", in_chns=1, class_num=4)
    fill_like_reference_init(list(model.named_parameters()))
    image, label = _zero_edge_case(60 if ours else 62)
    kw = {"inference": True} if ours else {}
    maps_got, maps_want = _resize_both_ways(
        monkeypatch, lambda: val_2D._predict_volume(image[0].numpy(), model, (64, 48), kw, 4))
    assert torch.is_tensor(maps_got) and maps_got.is_cuda and maps_got.dtype == torch.int64 and isinstance(maps_want, np.ndarray)
    assert maps_got.shape == maps_want.shape == (6, 78, 58)
    assert np.array_equal(maps_got.cpu().numpy(), maps_want)
    assert not maps_want[:, -1, :].any() and maps_want[:, -2, :].any()              # scipy's zero last row (64 -> 78)
    assert len(np.unique(maps_want)) > 1

    def run():
        if ours:
            return val_2D.test_single_volume_ours(image, label, model, classes=4, patch_size=(64, 48), slices_per_batch=4)
        return val_2D.test_single_volume(image, label, model, classes=4, patch_size=(64, 48), slices_per_batch=4)
    got, want = _resize_both_ways(monkeypatch, run)
    assert got == want and len(got) == 3
    assert [[type(v) for v in m] for m in got] == [[type(v) for v in m] for m in want]
    monkeypatch.setenv("ICL_VAL_METRICS", "host")                                  # a device prediction scored by the numpy path
    got_host_metrics, _ = _resize_both_ways(monkeypatch, run)
    assert got_host_metrics == want
