"""Surface metrics with a voxel spacing on the MI355X (kernels/metrics_surface.h): ops.seg_surface_metrics and the public functions of
icl_amd.val_3D / val_2D against the numpy / scipy restatement.  Cases, reference and the derived tolerances: tests/surface_ref.py (the
same cases run on the CPU emulator in test_surface_metrics_emu.py)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import surface_ref as sr  # noqa: E402

from icl_amd import ops, val_2D, val_3D  # noqa: E402
from icl_amd.utils.hashfill import fill_like_reference_init, synthetic_segmentation, synthetic_volume  # noqa: E402
from icl_amd.val_3D import cal_metric, cal_metric_multiclass, surface_metrics_multiclass  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from icl_amd import _lib
    assert _lib.lib_path().endswith("libicl_hip.so"), "GPU tests must run on the HIP library"
    return torch.device("cuda", 0)


def _check(gt, pred, nc, spacing, dev, tolerance=None):
    if tolerance is None:
        tolerance = 1.0 if sr.is_dyadic(spacing) else sr.NON_DYADIC_TOLERANCE
    counts, values = ops.seg_surface_metrics(torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev), nc, spacing, tolerance)
    assert counts.is_cuda and values.is_cuda and counts.dtype == torch.int64 and values.dtype == torch.float64
    counts, values = counts.cpu().tolist(), values.cpu().tolist()
    for c in range(1, nc):
        sr.check_record(counts[c - 1], values[c - 1], sr.Reference(gt, pred, c, spacing), spacing, tolerance)
    return counts, values


@pytest.mark.parametrize("spacing", sr.DYADIC + [sr.NON_DYADIC])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_overlapping_ellipsoids(dev, seed, spacing):
    gt, pred = sr.ellipsoids(seed)
    counts, values = _check(gt, pred, 2, spacing, dev)
    if spacing == (1.0, 1.0, 1.0):      # the floating path at unit spacing against the integers of the integer path
        g, p = torch.from_numpy(gt).to(dev), torch.from_numpy(pred).to(dev)
        rec = ops.seg_metrics(p, g, 2).cpu().tolist()[0]
        assert counts[0][:3] == rec[:3] and counts[0][3] + counts[0][4] == rec[3]
        assert values[0][0] == rec[4] and values[0][1] == rec[5]
        got, want = cal_metric_multiclass(g, p, 2, voxelspacing=(1, 1, 1)), cal_metric_multiclass(g, p, 2)
        assert got == want and [type(v) for v in got[0]] == [type(v) for v in want[0]]


@pytest.mark.parametrize("spacing", [(1.5, 1.5, 2.0), sr.NON_DYADIC])
def test_ellipsoids_48x56x40(dev, spacing):
    """Several hundred workgroups per pass and one partial per workgroup in the reduction."""
    gt, pred = sr.ellipsoids(7, (48, 56, 40))
    _check(gt, pred, 2, spacing, dev)


def test_anisotropy_changes_the_nearest_feature(dev):
    from scipy.ndimage import distance_transform_edt
    gt, pred = sr.anisotropy_pair()
    spacing = (10.0, 1.25, 1.25)
    q = tuple(int(v[0]) for v in np.nonzero(pred))
    iso = distance_transform_edt(gt == 0, return_distances=False, return_indices=True)[(slice(None),) + q]
    mm = distance_transform_edt(gt == 0, sampling=spacing, return_distances=False, return_indices=True)[(slice(None),) + q]
    assert tuple(iso) == (3, 21, 20) and tuple(mm) == (2, 20, 28)      # on the reference: another feature is the nearest
    counts, values = _check(gt, pred, 2, spacing, dev)
    assert values[0][2] == 100.0


@pytest.mark.parametrize("spacing", [(1.5, 1.5, 2.0), sr.NON_DYADIC])
@pytest.mark.parametrize("name", [n for n in sr.CASES if n != "anisotropy"])
def test_case(dev, name, spacing):
    gt, pred = sr.CASES[name]()
    counts, values = _check(gt, pred, 2, spacing, dev)
    if name == "identical_maps":
        assert values[0] == [0.0] * 6 and counts[0][5] == counts[0][3] and counts[0][6] == counts[0][4]
    if name == "single_voxels":
        assert counts[0][3:5] == [1, 1] and values[0][0] == values[0][1] == values[0][2] == values[0][3]


@pytest.mark.parametrize("near,far,spacing,sq", [
    ((3, 2, 1), (4, 0, 0), (0.5, 0.5, 0.5), (3.5, 4.0)),
    ((2, 9, 4), (0, 0, 8), (1.5, 1.5, 2.0), (255.25, 256.0)),
])
def test_ranks_part_at_a_power_of_two(dev, near, far, spacing, sq):
    """3.5 | 4.0 stands for the issue's 3.75 | 4.0, which no grid with dyadic spacings can produce (test_surface_metrics_emu.py says why);
    255.25 | 256.0 parts the two ranks in the select's top digit."""
    gt, pred = sr.three_points(near, far)
    assert (float(sr.pass_order_square(near, spacing)), float(sr.pass_order_square(far, spacing))) == sq
    counts, values = _check(gt, pred, 2, spacing, dev)
    assert (values[0][0], values[0][1]) == sq


def test_ranks_part_at_the_last_digit(dev):
    near, far = (7, 0, 2), (1, 2, 4)
    lo, hi = sr.pass_order_square(near, sr.NON_DYADIC), sr.pass_order_square(far, sr.NON_DYADIC)
    assert np.nextafter(lo, np.inf) == hi
    gt, pred = sr.three_points(near, far)
    counts, values = _check(gt, pred, 2, sr.NON_DYADIC, dev)
    assert values[0][0] == lo and values[0][1] == hi      # no fused multiply-add in the passes: the device forms the same two doubles


def test_four_classes_and_the_empty_mask_conventions(dev, monkeypatch):
    gt, pred = sr.four_class_maps()
    g, p = torch.from_numpy(gt).to(dev), torch.from_numpy(pred).to(dev)
    spacing = (1.5, 1.5, 2.0)
    _check(gt, pred, 5, spacing, dev)
    with monkeypatch.context() as m:      # the device run scores nothing on the host
        m.setattr(val_3D, "_surface_distances", _forbidden)
        recs = surface_metrics_multiclass(g, p, 5, spacing, 1.0)
        pairs = cal_metric_multiclass(g, p, 5, voxelspacing=spacing)
    monkeypatch.setenv("ICL_VAL_METRICS", "host")
    want = surface_metrics_multiclass(g, p, 5, spacing, 1.0)
    host = cal_metric_multiclass(g, p, 5, voxelspacing=spacing)
    ref = sr.Reference(gt, pred, 1, spacing)
    sr.check_dict(recs[0], ref, spacing, 1.0)
    sr.check_dict(want[0], ref, spacing, 1.0)
    one = {k: 373.128664 for k in recs[1]}
    one.update(dice=0, nsd=0.0)
    none = {k: 0 for k in recs[1]}
    none.update(dice=1, nsd=1.0)
    for got in (recs, want):
        assert got[1] == one and got[3] == one and got[2] == none
        for i in (1, 2, 3):
            assert [type(v) for v in got[i].values()] == [type(v) for v in (one if i != 2 else none).values()]
    assert pairs == host == [cal_metric(gt == c, pred == c, spacing) for c in range(1, 5)]
    assert [[type(v) for v in m] for m in pairs] == [[type(v) for v in m] for m in host]


def _forbidden(*args, **kwargs):
    raise AssertionError("the device run scored a class on the host")


def test_two_calls_are_bit_equal(dev):
    gt, pred = sr.ellipsoids(3, (48, 56, 40))
    g, p = torch.from_numpy(gt).to(dev), torch.from_numpy(pred).to(dev)
    a = ops.seg_surface_metrics(p, g, 2, sr.NON_DYADIC, 2.0)
    b = ops.seg_surface_metrics(p, g, 2, sr.NON_DYADIC, 2.0)
    assert torch.equal(a[0], b[0]) and a[1].cpu().numpy().tobytes() == b[1].cpu().numpy().tobytes()


def test_bad_arguments_are_refused(dev):
    a = torch.zeros((4, 4, 4), dtype=torch.int64, device=dev)
    for spacing in ((0.0, 1.0, 1.0), (1.0, -1.0, 1.0), (1.0, 1.0, float("nan")), (1.0, 1.0)):
        with pytest.raises(ValueError):
            ops.seg_surface_metrics(a, a, 2, spacing)
        with pytest.raises(ValueError):
            cal_metric_multiclass(a, a, 2, voxelspacing=spacing)
    with pytest.raises(ValueError):
        ops.seg_surface_metrics(a, a, 2, (1, 1, 1), -1.0)
    for nc in (1, 257):
        with pytest.raises(ValueError):
            ops.seg_surface_metrics(a, a, nc, (1, 1, 1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.seg_surface_metrics(a.cpu(), a.cpu(), 2, (1, 1, 1))


def test_all_case_base_with_a_spacing_device_equals_host(dev, monkeypatch):
    from icl_amd.networks.unet_3D import unet_3D
    from icl_amd.val_3D import test_all_case_base
    model = unet_3D(n_classes=3, in_channels=1, device=dev)
    fill_like_reference_init(list(model.named_parameters()))
    model.eval()
    cases = []
    for s in (0, 1):
        gt, _ = synthetic_segmentation((40, 48, 40), 3, 10 + s)
        cases.append((synthetic_volume((40, 48, 40), 20 + s).numpy() + gt.astype(np.float32), gt))
    run = lambda: test_all_case_base(model, "unet_3D", None, num_classes=3, patch_size=(32, 48, 32), stride_xy=8, stride_z=8,  # noqa: E731
                                     cases=list(cases), voxelspacing=(1.5, 1.5, 2.0))
    monkeypatch.setenv("ICL_VAL_METRICS", "host")
    want = run()
    monkeypatch.setenv("ICL_VAL_METRICS", "device")
    with monkeypatch.context() as m:
        m.setattr(val_3D, "cal_metric", _forbidden)
        got = run()
    assert got == want and len(got) == 2 and all(len(m) == 2 for m in got)      # dyadic spacing: bit-equal
    assert [type(v) for m in got for pair in m for v in pair] == [type(v) for m in want for pair in m for v in pair]


def test_single_volume_with_a_spacing_device_equals_host(dev, monkeypatch):
    from icl_amd.networks.net_factory import net_factory
    from icl_amd.val_2D import test_single_volume
    model = net_factory(net_type="unet", in_chns=1, class_num=4)
    fill_like_reference_init(list(model.named_parameters()))
    gt, _ = synthetic_segmentation((6, 80, 72), 4, 40)
    image = torch.from_numpy(synthetic_volume((6, 80, 72), 41).numpy() + gt.astype(np.float32)).unsqueeze(0)
    label = torch.from_numpy(gt).unsqueeze(0)
    run = lambda: test_single_volume(image, label, model, classes=4, patch_size=(64, 64), voxelspacing=(10, 1.25, 1.25))  # noqa: E731
    monkeypatch.setenv("ICL_VAL_METRICS", "host")
    want = run()
    monkeypatch.setenv("ICL_VAL_METRICS", "device")
    with monkeypatch.context() as m:
        m.setattr(val_2D, "calculate_metric_percase", _forbidden)
        got = run()
    assert got == want and len(got) == 3
