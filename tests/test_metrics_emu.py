"""CPU checks of the validation-metric kernels (icl_amd/csrc/kernels/metrics.h) through tests/hipemu and the C ABI.

Every case asserts EQUALITY with the numpy restatement of the reference metric (icl_amd.val_3D.cal_metric: scipy's erosion and exact
Euclidean distance transform, np.percentile): same values, same types, bit-equal floats.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hipemu"))
from build_emu import build_emu  # noqa: E402

from icl_amd import _lib, ops  # noqa: E402
from icl_amd.utils.hashfill import synthetic_segmentation  # noqa: E402
from icl_amd.val_3D import _cal_metric_kernels, _upload_label, cal_metric, cal_metric_multiclass, hd95_from_order_stats  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def emu_library():
    _lib._use_library_for_tests(build_emu(), host_pointers=True)
    yield
    _lib._use_library_for_tests(None)


def _check(gt, pred, nc):
    """The kernel path on host tensors (emulator) against cal_metric per class: values, types, bit patterns."""
    got = _cal_metric_kernels(torch.from_numpy(np.ascontiguousarray(gt)), torch.from_numpy(np.ascontiguousarray(pred)), nc)
    want = [cal_metric(gt == c, pred == c) for c in range(1, nc)]
    assert len(got) == len(want)
    for c, (g, w) in enumerate(zip(got, want), 1):
        assert g == w, (c, g, w)
        assert [type(v) for v in g] == [type(v) for v in w], (c, g, w)
    return got


def _blob(shape, center, radii, rng=None, speckle=0.0):
    idx = np.indices(shape).astype(np.float64)
    r = sum(((idx[i] - center[i]) / radii[i]) ** 2 for i in range(3))
    m = r <= 1.0
    if rng is not None and speckle:
        m ^= rng.random(shape) < speckle
    return m


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_overlapping_blobs_odd_volume(seed):
    rng = np.random.default_rng(seed)
    shape = (19, 23, 17)
    gt = _blob(shape, (9, 11, 8), (6, 8, 5), rng, 0.03).astype(np.uint8)
    pred = _blob(shape, (10, 12, 7), (5, 7, 6), rng, 0.03).astype(np.int64)
    got = _check(gt, pred, 2)
    assert 0 < got[0][0] < 1 and got[0][1] > 0


def test_objects_touching_the_faces():
    shape = (12, 15, 10)
    gt = np.zeros(shape, np.uint8)
    gt[:5, :, :4] = 1                     # slab on three faces
    pred = np.zeros(shape, np.int64)
    pred[:, 10:, :] = 1                   # slab on five faces
    pred[0, 0, 0] = 1
    _check(gt, pred, 2)


def test_single_voxel_against_a_large_ground_truth():
    shape = (16, 14, 18)
    gt = _blob(shape, (8, 7, 9), (7, 6, 8)).astype(np.int64)
    pred = np.zeros(shape, np.uint8)
    pred[3, 4, 5] = 1
    _check(gt, pred, 2)


def test_identical_masks_give_zero():
    rng = np.random.default_rng(5)
    m = _blob((13, 11, 9), (6, 5, 4), (5, 4, 3), rng, 0.05).astype(np.int64)
    got = _check(m, m, 2)
    assert got[0] == (1.0, 0.0)


def test_prediction_strictly_inside_the_ground_truth():
    shape = (17, 17, 17)
    gt = _blob(shape, (8, 8, 8), (7, 7, 7)).astype(np.uint8)
    pred = _blob(shape, (8, 8, 8), (3, 4, 2)).astype(np.int64)
    _check(gt, pred, 2)


def test_features_confined_to_one_corner():
    shape = (20, 18, 22)
    gt = np.zeros(shape, np.uint8)
    gt[:3, :2, :3] = 1                    # most lines of every pass hold no feature
    pred = np.zeros(shape, np.int64)
    pred[15:, 14:, 17:] = 1
    pred[10, 2, 20] = 1
    _check(gt, pred, 2)


def test_distances_beyond_the_lds_histogram():
    """Squared distances >= 1024 go to the global histogram bins (39^2 = 1521 here)."""
    shape = (40, 3, 3)
    gt = np.zeros(shape, np.uint8)
    gt[:2] = 1
    pred = np.zeros(shape, np.int64)
    pred[-2:] = 1
    pred[20, 1, 1] = 1
    got = _check(gt, pred, 2)
    assert got[0][1] > 32


@pytest.mark.parametrize("seed", [0, 1])
def test_prediction_scattered_over_the_volume(seed):
    """Feature and query borders in very different boxes (a compact ground truth, a prediction speckled everywhere): every pass runs
    on the F / Q sub-boxes and the pruned outward scans."""
    gt, pred = synthetic_segmentation((21, 19, 17), 4, seed, speckle=0.05, scatter=0.03)
    _check(gt, pred, 4)


@pytest.mark.parametrize("shape", [(1, 9, 11), (7, 1, 6), (8, 5, 1), (2, 9, 7), (6, 2, 2), (1, 1, 13), (2, 2, 2)])
def test_axes_of_length_one_and_two(shape):
    rng = np.random.default_rng(sum(shape))
    gt = (rng.random(shape) < 0.4).astype(np.uint8)
    pred = (rng.random(shape) < 0.5).astype(np.int64)
    gt.flat[0] = 1
    pred.flat[-1] = 1
    _check(gt, pred, 2)


def test_multiclass_map_with_absent_classes():
    rng = np.random.default_rng(11)
    shape = (15, 13, 11)
    gt = np.zeros(shape, np.uint8)
    pred = np.zeros(shape, np.int64)
    gt[_blob(shape, (5, 5, 5), (4, 4, 3))] = 1
    pred[_blob(shape, (6, 5, 4), (4, 3, 3))] = 1
    gt[_blob(shape, (10, 9, 7), (3, 3, 3))] = 2              # class 2 only in gt
    pred[_blob(shape, (10, 3, 8), (2, 2, 2))] = 3            # class 3 only in pred
    gt[_blob(shape, (3, 10, 2), (2, 2, 2), rng, 0.05)] = 5    # class 5 in both, noisy
    pred[_blob(shape, (3, 11, 3), (2, 2, 2), rng, 0.05)] = 5
    gt[0, 0, 0] = 7                                          # labels >= num_classes belong to no class
    got = _check(gt, pred, 7)                                 # class 4 and 6 absent from both
    assert got[1] == (0, 373.128664) and got[2] == (0, 373.128664) and got[3] == (1, 0) and got[5] == (1, 0)
    assert isinstance(got[3][0], int) and isinstance(got[3][1], int)


def test_four_dimensional_maps_of_the_amos_path():
    """test_all_case_amos scores [1, D, H, W] maps: under the 4-D erosion every voxel of a class is a surface voxel."""
    rng = np.random.default_rng(3)
    shape = (1, 9, 10, 8)
    gt = (rng.random(shape) * 3).astype(np.int64)
    pred = (rng.random(shape) * 3).astype(np.uint8)
    _check(gt, pred, 3)


def test_records_and_multiclass_entry_on_host_tensors():
    rng = np.random.default_rng(8)
    gt = torch.from_numpy((rng.random((9, 8, 7)) * 4).astype(np.int64))
    pred = torch.from_numpy((rng.random((9, 8, 7)) * 4).astype(np.uint8))
    rec = ops.seg_metrics(pred, gt, 4)
    assert rec.shape == (3, 6) and rec.dtype == torch.int64
    g, p = gt.numpy(), pred.numpy()
    for c in range(1, 4):
        assert rec[c - 1, 0] == (p == c).sum() and rec[c - 1, 1] == (g == c).sum() and rec[c - 1, 2] == ((p == c) & (g == c)).sum()
    # host tensors take the numpy path in the public entry (the device path applies to HIP tensors only)
    assert cal_metric_multiclass(gt, pred, 4) == [cal_metric(gt == c, pred == c) for c in range(1, 4)]


def test_bad_arguments_are_refused():
    a = torch.zeros((4, 4, 4), dtype=torch.int64)
    with pytest.raises(ValueError):
        ops.seg_metrics(a, torch.zeros((4, 4, 5), dtype=torch.int64), 2)
    with pytest.raises(TypeError):
        ops.seg_metrics(a.float(), a, 2)
    with pytest.raises(TypeError):
        ops.seg_metrics(a.int(), a, 2)
    with pytest.raises(ValueError):
        ops.seg_metrics(a[0], a[0], 2)
    with pytest.raises(ValueError):
        ops.seg_metrics(a, a, 1)


def test_percentile_interpolation_helper():
    rng = np.random.default_rng(0)
    for n in range(2, 3001):
        sq = np.sort(rng.integers(0, 5000, size=n))
        if n % 3 == 0:
            sq = np.sort(rng.integers(0, 4, size=n))                 # many ties
        k0 = int(np.floor((n - 1) * 0.95))
        want = float(np.percentile(np.sqrt(sq.astype(np.float64)), 95))
        got = hd95_from_order_stats(n, int(sq[k0]), int(sq[k0 + 1]))
        assert got == want, (n, got, want)


def test_label_upload_dtypes():
    """Host label maps the device path takes: integer and bool maps, floating maps holding only integers (MONAI's float32 labels); a
    floating map with any other value stays on the numpy path."""
    f = np.array([[[0.0, 1.0], [2.0, 3.0]]], np.float32)
    t = _upload_label(f, "cpu")
    assert t.dtype == torch.uint8 and t.tolist() == [[[0, 1], [2, 3]]]
    t = _upload_label(torch.from_numpy(f * 100), "cpu")
    assert t.dtype == torch.int64 and int(t.max()) == 300
    assert _upload_label(-f, "cpu").dtype == torch.int64
    assert _upload_label(f + 0.5, "cpu") is None
    g = f.copy()
    g[0, 0, 0] = np.nan
    assert _upload_label(g, "cpu") is None
    assert _upload_label(f.astype(np.int16), "cpu").dtype == torch.int64
    assert _upload_label(f.astype(np.uint8), "cpu").dtype == torch.uint8
    assert _upload_label(np.array(["a"]), "cpu") is None


# the sizes that the library of commit ca1119d2aa3a5921954c12ced9f9332573bd19a7 (the parent of the one that put the workspace carver into the
# launchers) returns, recorded from its emulation build: the layout of the workspace has not moved
@pytest.mark.parametrize("shape, nc, nbytes", [((1, 1, 1), 2, 2048), ((5, 7, 9), 3, 5120), ((3, 300, 2), 256, 1022720), ((96, 96, 96), 16, 8994304)])
def test_workspace_size_is_that_of_the_earlier_layout(shape, nc, nbytes):
    assert _lib.lib().icl_seg_metrics_ws_bytes(*shape, nc) == nbytes
