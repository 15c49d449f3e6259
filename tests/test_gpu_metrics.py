"""Validation Dice / HD95 on the MI355X (kernels/metrics.h): the device path equals the numpy restatement (icl_amd.val_3D.cal_metric)
value for value and bit for bit, on its own and inside the validation loops of the trainers (ICL_VAL_METRICS=device vs =host)."""
import numpy as np
import pytest
import torch

from icl_amd import val_2D, val_3D
from icl_amd.utils.hashfill import fill_like_reference_init, synthetic_segmentation, synthetic_volume
from icl_amd.val_3D import cal_metric, cal_metric_multiclass

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from icl_amd import _lib
    assert _lib.lib_path().endswith("libicl_hip.so"), "GPU tests must run on the HIP library"
    return torch.device("cuda", 0)


def _check(gt, pred, nc, dev):
    got = cal_metric_multiclass(torch.from_numpy(gt).to(dev), torch.from_numpy(pred).to(dev), nc)
    want = [cal_metric(gt == c, pred == c) for c in range(1, nc)]
    assert got == want
    assert [[type(v) for v in m] for m in got] == [[type(v) for v in m] for m in want]
    return got


def test_one_class_ellipsoids_240x240x155(dev):
    gt, pred = synthetic_segmentation((240, 240, 155), 2, 1, speckle=0.02)
    got = _check(gt, pred, 2, dev)
    assert 0 < got[0][0] < 1 and got[0][1] > 0


def test_fifteen_classes_256x256x128(dev):
    gt, pred = synthetic_segmentation((256, 256, 128), 16, 2)
    got = _check(gt, pred, 16, dev)
    assert all(isinstance(m[0], float) for m in got)


def test_empty_classes_140x170x139(dev):
    gt, pred = synthetic_segmentation((140, 170, 139), 6, 3)
    gt[gt == 2] = 0          # class 2: prediction only
    pred[pred == 3] = 0      # class 3: ground truth only
    gt[gt == 4] = 0          # class 4: neither
    pred[pred == 4] = 0
    got = _check(gt, pred, 7, dev)        # class 6: absent from both maps as well
    assert got[1] == (0, 373.128664) and got[2] == (0, 373.128664) and got[3] == (1, 0) and got[5] == (1, 0)


@pytest.mark.parametrize("pred_dtype,gt_dtype", [(np.uint8, np.uint8), (np.uint8, np.int64), (np.int64, np.uint8), (np.int64, np.int64)])
def test_label_dtypes(dev, pred_dtype, gt_dtype):
    gt, pred = synthetic_segmentation((64, 48, 40), 4, 4)
    _check(gt.astype(gt_dtype), pred.astype(pred_dtype), 4, dev)


def _host_metric_forbidden(*args, **kwargs):
    raise AssertionError("the device run scored a class on the host")


def _both_ways(monkeypatch, fn, host_metric):
    """fn() under ICL_VAL_METRICS=host, then under =device with the host scoring function (module, name) made to fail if called: the
    device run must take the device path."""
    monkeypatch.setenv("ICL_VAL_METRICS", "host")
    want = fn()
    monkeypatch.setenv("ICL_VAL_METRICS", "device")
    with monkeypatch.context() as m:
        m.setattr(host_metric[0], host_metric[1], _host_metric_forbidden)
        got = fn()
    return got, want


def test_all_case_base_device_equals_host(dev, monkeypatch):
    from icl_amd.networks.unet_3D import unet_3D
    from icl_amd.val_3D import test_all_case_base
    model = unet_3D(n_classes=3, in_channels=1, device=dev)
    fill_like_reference_init(list(model.named_parameters()))
    model.eval()
    cases = []
    for s in (0, 1):
        gt, _ = synthetic_segmentation((70, 84, 66), 3, 10 + s)
        img = synthetic_volume((70, 84, 66), 20 + s).numpy() + gt.astype(np.float32)
        cases.append((img, gt))
    got, want = _both_ways(monkeypatch, lambda: test_all_case_base(model, "unet_3D", None, num_classes=3, patch_size=(48, 64, 64),
                                                                 stride_xy=32, stride_z=24, cases=list(cases)), (val_3D, "cal_metric"))
    assert got == want and len(got) == 2 and all(len(m) == 2 for m in got)


def test_all_case_amos_device_equals_host(dev, monkeypatch):
    from icl_amd.networks.unet_3D import unet_3D
    from icl_amd.val_3D import test_all_case_amos
    model = unet_3D(n_classes=4, in_channels=1, device=dev)
    fill_like_reference_init(list(model.named_parameters()))
    gt, _ = synthetic_segmentation((100, 98, 97), 4, 30)
    vol = torch.from_numpy(synthetic_volume((100, 98, 97), 31).numpy() + gt.astype(np.float32)).view(1, 1, 100, 98, 97)
    lab = torch.from_numpy(gt.astype(np.int64)).view(1, 1, 100, 98, 97)
    got, want = _both_ways(monkeypatch, lambda: test_all_case_amos(model, "unet_3D", [{"image": vol, "label": lab}], num_classes=4),
                           (val_3D, "cal_metric"))
    assert got == want and len(got) == 3


def test_all_case_amos_float_labels_take_the_device_path(dev, monkeypatch):
    """MONAI's LoadImaged yields float32 labels: [1, 1, D, H, W] float32 holding integers are scored on the device, equal to the host."""
    from icl_amd.networks.unet_3D import unet_3D
    from icl_amd.val_3D import test_all_case_amos
    model = unet_3D(n_classes=4, in_channels=1, device=dev)
    fill_like_reference_init(list(model.named_parameters()))
    gt, _ = synthetic_segmentation((100, 98, 97), 4, 32)
    vol = torch.from_numpy(synthetic_volume((100, 98, 97), 33).numpy() + gt.astype(np.float32)).view(1, 1, 100, 98, 97)
    lab = torch.from_numpy(gt.astype(np.float32)).view(1, 1, 100, 98, 97)
    got, want = _both_ways(monkeypatch, lambda: test_all_case_amos(model, "unet_3D", [{"image": vol, "label": lab}], num_classes=4),
                           (val_3D, "cal_metric"))
    assert got == want and len(got) == 3


def test_prediction_scattered_over_the_volume(dev):
    """An early-training prediction: 2 % of the voxels carry a random class, so every class's border spans the whole volume."""
    gt, pred = synthetic_segmentation((128, 112, 96), 16, 5, scatter=0.02)
    _check(gt, pred, 16, dev)


def test_class_counts_outside_the_kernel_range_take_the_numpy_path(dev):
    gt, pred = synthetic_segmentation((24, 20, 16), 3, 6)
    g, p = torch.from_numpy(gt).to(dev), torch.from_numpy(pred).to(dev)
    assert cal_metric_multiclass(g, p, 1) == []
    assert cal_metric_multiclass(g, p, 300) == [cal_metric(gt == c, pred == c) for c in range(1, 300)]


def test_single_volume_ours_device_equals_host(dev, monkeypatch):
    from icl_amd.networks.net_factory import net_factory
    from icl_amd.val_2D import test_single_volume_ours
    model = net_factory(net_type="icl_unet", in_chns=1, class_num=4)
    fill_like_reference_init(list(model.named_parameters()))
    gt, _ = synthetic_segmentation((6, 80, 72), 4, 40)
    image = torch.from_numpy(synthetic_volume((6, 80, 72), 41).numpy() + gt.astype(np.float32)).unsqueeze(0)
    label = torch.from_numpy(gt).unsqueeze(0)
    got, want = _both_ways(monkeypatch, lambda: test_single_volume_ours(image, label, model, classes=4, patch_size=(64, 64)),
                           (val_2D, "calculate_metric_percase"))
    assert got == want and len(got) == 3
