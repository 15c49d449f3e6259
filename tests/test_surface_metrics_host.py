"""Host logic of the surface metrics with a voxel spacing (no device): the numpy / scipy restatements, the keyword defaults of the public
functions (unchanged values and types without a spacing), and the way the spacing reaches the metric from the four validation loops."""
import numpy as np
import pytest
import torch
from scipy.ndimage import binary_erosion, distance_transform_edt, generate_binary_structure

from icl_amd import val_2D, val_3D
from icl_amd.val_3D import (binary_asd, binary_assd, binary_dice, binary_hd, binary_hd95, binary_nsd, cal_metric, cal_metric_multiclass,
                            surface_metrics_multiclass)


def _blob(shape, center, radii):
    idx = np.indices(shape).astype(np.float64)
    return sum(((idx[i] - center[i]) / radii[i]) ** 2 for i in range(len(shape))) <= 1.0


def _maps(shape=(12, 14, 10), classes=3):
    gt = np.zeros(shape, np.uint8)
    pred = np.zeros(shape, np.int64)
    c = [s / 2 for s in shape]
    gt[_blob(shape, (c[0] - 1, c[1], c[2]), (shape[0] / 3, shape[1] / 3, shape[2] / 3))] = 1
    pred[_blob(shape, (c[0], c[1] + 1, c[2]), (shape[0] / 3.5, shape[1] / 3, shape[2] / 2.8))] = 1
    if classes > 2:
        gt[:2, :3, :2] = 2
        pred[:3, :2, :2] = 2
    return gt, pred


def _distances(a, b, sampling=None):
    """Written out here on scipy alone: the border voxels of a (connectivity-1 erosion) and their distance to the border of b."""
    fp = generate_binary_structure(a.ndim, 1)
    ab = a ^ binary_erosion(a, structure=fp, iterations=1)
    bb = b ^ binary_erosion(b, structure=fp, iterations=1)
    return distance_transform_edt(~bb, sampling=sampling)[ab]


def _pair(g, p, sampling=None):
    """(dice, hd95) of two non-empty masks as the parent commit forms them, the spacing passed to scipy."""
    d = np.hstack((_distances(p, g, sampling), _distances(g, p, sampling)))
    return 2.0 * np.count_nonzero(p & g) / float(np.count_nonzero(p) + np.count_nonzero(g)), float(np.percentile(d, 95))


class _RoundNet(torch.nn.Module):
    """logits[:, k] = -(x - k)^2: the arg-max is the input rounded to the nearest class — the prediction is the image."""

    def __init__(self, classes):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.classes = classes

    def forward(self, x, inference=False):
        return torch.cat([-(x - k) ** 2 for k in range(self.classes)], dim=1)


def test_restatements_at_unit_spacing_equal_the_plain_hd95():
    gt, pred = _maps()
    g, p = gt == 1, pred == 1
    plain = binary_hd95(p, g)
    assert plain == _pair(g, p)[1]
    for sp in ((1, 1, 1), 1, 1.0, np.ones(3), [1.0, 1.0, 1.0]):
        assert binary_hd95(p, g, voxelspacing=sp) == plain
    a, b = _distances(p, g), _distances(g, p)
    assert binary_hd(p, g) == binary_hd(p, g, (1, 1, 1)) == float(max(a.max(), b.max()))
    assert binary_asd(p, g) == binary_asd(p, g, 1.0) == float(a.mean()) and binary_asd(g, p) == float(b.mean())
    assert binary_assd(p, g) == float(np.mean((a.mean(), b.mean())))
    assert binary_nsd(p, g, 1.0) == binary_nsd(p, g, 1.0, (1, 1, 1)) == float(((a <= 1).sum() + (b <= 1).sum()) / (len(a) + len(b)))
    assert binary_nsd(p, p, 0.0) == 1.0


def test_restatements_with_a_spacing():
    gt, pred = _maps()
    g, p = gt == 1, pred == 1
    sp = (10, 1.25, 1.25)
    a, b = _distances(p, g, sp), _distances(g, p, sp)
    assert binary_hd95(p, g, sp) == float(np.percentile(np.hstack((a, b)), 95)) != binary_hd95(p, g)
    assert binary_hd(p, g, sp) == float(max(a.max(), b.max()))
    assert binary_asd(p, g, sp) == float(a.mean()) and binary_asd(g, p, sp) == float(b.mean())
    assert binary_assd(p, g, sp) == float(np.mean((a.mean(), b.mean())))
    assert binary_nsd(p, g, 2.5, sp) == float(((a <= 2.5).sum() + (b <= 2.5).sum()) / (len(a) + len(b)))
    # a scalar is broadcast, as scipy's _normalize_sequence does
    assert binary_hd95(p, g, 2.0) == binary_hd95(p, g, (2.0, 2.0, 2.0)) == 2.0 * binary_hd95(p, g)
    rec = surface_metrics_multiclass(gt, pred, 2, sp, 2.5)[0]
    assert rec == {"dice": binary_dice(p, g), "hd95": binary_hd95(p, g, sp), "hd": binary_hd(p, g, sp), "assd": binary_assd(p, g, sp),
                   "asd_pred_gt": binary_asd(p, g, sp), "asd_gt_pred": binary_asd(g, p, sp), "nsd": binary_nsd(p, g, 2.5, sp)}
    assert surface_metrics_multiclass(gt, pred, 2)[0]["hd95"] == binary_hd95(p, g)      # None: unit spacing, tolerance 1.0


def test_four_dimensional_maps_take_the_spacing_on_their_last_three_axes():
    gt, pred = _maps((7, 8, 6))
    g, p = (gt == 1)[None], (pred == 1)[None]
    assert binary_hd95(p, g, (1.5, 1.5, 2.0)) == _pair(g, p, (1.0, 1.5, 1.5, 2.0))[1]
    with pytest.raises(ValueError):
        binary_hd95(p[0, 0], g[0, 0], (1.5, 1.5, 2.0))      # a 2-D map has no three axes to space
    with pytest.raises(ValueError):
        binary_hd95(np.stack((p[0], p[0])), np.stack((g[0], g[0])), (1.5, 1.5, 2.0))


@pytest.mark.parametrize("bad", [0, -1.0, float("nan"), float("inf"), (1.0, 1.0), (1.0, 1.0, 1.0, 1.0), (1.0, 0.0, 1.0), (1.0, -2.0, 1.0),
                                 (1.0, float("nan"), 1.0), "1", ((1, 1, 1),), ()])
def test_a_bad_spacing_is_a_value_error_everywhere(bad):
    gt, pred = _maps()
    for call in (lambda: binary_hd95(pred == 1, gt == 1, bad), lambda: binary_nsd(pred == 1, gt == 1, 1.0, bad),
                 lambda: cal_metric(gt == 1, pred == 1, bad), lambda: cal_metric_multiclass(gt, pred, 3, bad),
                 lambda: cal_metric_multiclass(gt, pred, 3, voxelspacing=bad), lambda: surface_metrics_multiclass(gt, pred, 3, bad),
                 lambda: val_3D.test_all_case_base(_RoundNet(3), "unet_3D", None, num_classes=3, cases=[], voxelspacing=bad),
                 lambda: val_3D.test_all_case_amos(_RoundNet(3), "unet_3D", [], num_classes=3, voxelspacing=bad),
                 lambda: val_2D.calculate_metric_percase(pred == 1, gt == 1, bad)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError):
        surface_metrics_multiclass(gt, pred, 3, (1, 1, 1), tolerance=-1.0)
    with pytest.raises(ValueError):
        binary_nsd(pred == 1, gt == 1, float("nan"))


def test_keyword_defaults_leave_the_metric_functions_as_they_were():
    gt, pred = _maps()
    want = [_pair(gt == c, pred == c) for c in (1, 2)]
    assert [cal_metric(gt == c, pred == c) for c in (1, 2)] == want
    got = cal_metric_multiclass(gt, pred, 5)
    assert got == want + [(1, 0), (1, 0)]
    assert [type(v) for m in got for v in m] == [float, float, float, float, int, int, int, int]
    only_gt = np.where(pred == 2, 0, pred)
    got = cal_metric_multiclass(gt, only_gt, 3)
    assert got[1] == (0, 373.128664) and isinstance(got[1][0], int) and isinstance(got[1][1], float)
    assert cal_metric_multiclass(torch.from_numpy(gt), torch.from_numpy(pred), 3) == want
    assert val_2D.calculate_metric_percase(pred == 1, gt == 1) == want[0]


def test_empty_mask_conventions_with_a_spacing():
    gt, pred = _maps()
    only_gt = np.where(pred == 2, 0, pred)
    sp = (1.5, 1.5, 2.0)
    got = cal_metric_multiclass(gt, only_gt, 4, voxelspacing=sp)
    assert got == [_pair(gt == 1, pred == 1, sp), (0, 373.128664), (1, 0)]
    assert [type(v) for v in got[1]] == [int, float] and [type(v) for v in got[2]] == [int, int]
    recs = surface_metrics_multiclass(gt, only_gt, 4, sp)
    assert recs[1] == {"dice": 0, "hd95": 373.128664, "hd": 373.128664, "assd": 373.128664, "asd_pred_gt": 373.128664,
                       "asd_gt_pred": 373.128664, "nsd": 0.0}
    assert recs[2] == {"dice": 1, "hd95": 0, "hd": 0, "assd": 0, "asd_pred_gt": 0, "asd_gt_pred": 0, "nsd": 1.0}
    assert isinstance(recs[1]["dice"], int) and isinstance(recs[2]["hd"], int) and isinstance(recs[2]["nsd"], float)


def _cases_3d():
    out = []
    for shift in (0, 1):
        gt, pred = _maps((12, 14, 10))
        pred = np.roll(pred, shift, axis=2)
        out.append((pred.astype(np.float32), gt))      # the image IS the prediction (_RoundNet)
    return out


def test_all_case_base_default_and_spacing():
    net = _RoundNet(3)
    cases = _cases_3d()
    run = lambda **kw: val_3D.test_all_case_base(net, "unet_3D", None, num_classes=3, patch_size=(12, 14, 10), stride_xy=8, stride_z=8,  # noqa: E731
                                                 cases=list(cases), **kw)
    want = [[_pair(gt == c, img.astype(np.int64) == c) for img, gt in cases] for c in (1, 2)]
    assert run() == want == run(voxelspacing=None)
    sp = (1.5, 1.5, 2.0)
    want_sp = [[_pair(gt == c, img.astype(np.int64) == c, sp) for img, gt in cases] for c in (1, 2)]
    assert run(voxelspacing=sp) == want_sp != want
    assert [type(v) for m in run(voxelspacing=sp) for pair in m for v in pair] == [float] * 8


def test_all_case_amos_default_and_spacing():
    net = _RoundNet(3)
    gt, pred = _maps((12, 14, 10))
    loader = [{"image": torch.from_numpy(pred.astype(np.float32))[None, None], "label": torch.from_numpy(gt.astype(np.int64))[None, None]}]
    # the loop scores [1, D, H, W] maps (4-D erosion: every voxel of a class is a border voxel)
    want = [[_pair((gt == c)[None], (pred == c)[None])] for c in (1, 2)]
    assert val_3D.test_all_case_amos(net, "unet_3D", loader, num_classes=3) == want
    sp = (1.5, 1.5, 2.0)
    want_sp = [[_pair((gt == c)[None], (pred == c)[None], (1.0,) + sp)] for c in (1, 2)]
    assert val_3D.test_all_case_amos(net, "unet_3D", loader, num_classes=3, voxelspacing=sp) == want_sp != want


@pytest.mark.parametrize("fn", ["test_single_volume", "test_single_volume_ours"])
def test_single_volume_default_and_spacing(fn):
    net = _RoundNet(3)
    gt, pred = _maps((5, 16, 12))
    image = torch.from_numpy(pred.astype(np.float32))[None]
    label = torch.from_numpy(gt)[None]
    run = getattr(val_2D, fn)
    kw = {"classes": 3, "patch_size": (16, 12)}
    want = [_pair(pred == c, gt == c) for c in (1, 2)]
    assert run(image, label, net, **kw) == want == run(image, label, net, voxelspacing=None, **kw)
    sp = (10, 1.25, 1.25)
    want_sp = [_pair(pred == c, gt == c, sp) for c in (1, 2)]
    assert run(image, label, net, voxelspacing=sp, **kw) == want_sp != want


def test_compat_modules_re_export_the_new_names():
    import importlib
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "compat"))
    try:
        for name in ("val_3D", "val_2D"):
            sys.modules.pop(name, None)
        m3, m2 = importlib.import_module("val_3D"), importlib.import_module("val_2D")
        assert m3.surface_metrics_multiclass is surface_metrics_multiclass and m3.binary_nsd is binary_nsd and m3.binary_assd is binary_assd
        assert m2.test_single_volume is val_2D.test_single_volume
    finally:
        sys.path.remove(os.path.join(root, "compat"))
        for name in ("val_3D", "val_2D"):
            sys.modules.pop(name, None)
