"""CPU checks of the surface-metric kernels (icl_amd/csrc/kernels/metrics_surface.h) through tests/hipemu and the C ABI, against the
numpy / scipy restatement (icl_amd.val_3D._surface_distances with a spacing, np.percentile, .mean()).  Cases, reference and the
derived tolerances: tests/surface_ref.py."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hipemu"))
sys.path.insert(0, HERE)
from build_emu import build_emu  # noqa: E402

import surface_ref as sr  # noqa: E402
from icl_amd import _lib, ops  # noqa: E402
from icl_amd.val_3D import (_cal_metric_kernels, _cal_metric_surface_kernels, _surface_records_kernels, cal_metric,  # noqa: E402
                            cal_metric_multiclass, surface_metrics_multiclass)


@pytest.fixture(scope="module", autouse=True)
def emu_library():
    _lib._use_library_for_tests(build_emu(), host_pointers=True)
    yield
    _lib._use_library_for_tests(None)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _run(gt, pred, nc, spacing, tolerance=1.0):
    counts, values = ops.seg_surface_metrics(_t(pred), _t(gt), nc, spacing, tolerance)
    assert counts.shape == (nc - 1, 7) and counts.dtype == torch.int64
    assert values.shape == (nc - 1, 6) and values.dtype == torch.float64
    return counts.tolist(), values.tolist()


def _check(gt, pred, nc, spacing, tolerance=None):
    if tolerance is None:
        tolerance = 1.0 if sr.is_dyadic(spacing) else sr.NON_DYADIC_TOLERANCE
    counts, values = _run(gt, pred, nc, spacing, tolerance)
    for c in range(1, nc):
        sr.check_record(counts[c - 1], values[c - 1], sr.Reference(gt, pred, c, spacing), spacing, tolerance)
    return counts, values


@pytest.mark.parametrize("spacing", sr.DYADIC + [sr.NON_DYADIC])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_overlapping_ellipsoids(seed, spacing):
    gt, pred = sr.ellipsoids(seed)
    counts, values = _check(gt, pred, 2, spacing)
    assert values[0][0] > 0 and counts[0][3] > 100
    if spacing == (1.0, 1.0, 1.0):      # the floating path at unit spacing against the integers of the integer path
        rec = ops.seg_metrics(_t(pred), _t(gt), 2).tolist()[0]
        assert counts[0][:3] == rec[:3] and counts[0][3] + counts[0][4] == rec[3]
        assert values[0][0] == rec[4] and values[0][1] == rec[5]
        assert _cal_metric_surface_kernels(_t(gt), _t(pred), 2, spacing) == _cal_metric_kernels(_t(gt), _t(pred), 2)


def test_anisotropy_changes_the_nearest_feature():
    from scipy.ndimage import distance_transform_edt
    gt, pred = sr.anisotropy_pair()
    spacing = (10.0, 1.25, 1.25)
    q = tuple(int(v[0]) for v in np.nonzero(pred))
    iso = distance_transform_edt(gt == 0, return_distances=False, return_indices=True)[(slice(None),) + q]
    mm = distance_transform_edt(gt == 0, sampling=spacing, return_distances=False, return_indices=True)[(slice(None),) + q]
    assert tuple(iso) == (3, 21, 20) and tuple(mm) == (2, 20, 28)      # on the reference: another feature is the nearest
    counts, values = _check(gt, pred, 2, spacing)
    assert values[0][2] == 100.0      # dP -> dG: 8 pixels of 1.25 mm, not the slice neighbour at sqrt(101.5625) mm
    _check(gt, pred, 2, (1.0, 1.0, 1.0))


@pytest.mark.parametrize("spacing", [(1.5, 1.5, 2.0), sr.NON_DYADIC])
@pytest.mark.parametrize("name", [n for n in sr.CASES if n != "anisotropy"])
def test_case(name, spacing):
    gt, pred = sr.CASES[name]()
    counts, values = _check(gt, pred, 2, spacing)
    if name == "identical_maps":      # every key is zero: both ranks in one bucket through every digit
        assert values[0] == [0.0] * 6 and counts[0][5] == counts[0][3] and counts[0][6] == counts[0][4]
    if name == "single_voxels":       # n = 2: ranks 0 and 1
        assert counts[0][3:5] == [1, 1] and values[0][0] == values[0][1] == values[0][2] == values[0][3]


@pytest.mark.parametrize("near,far,spacing,sq", [
    ((3, 2, 1), (4, 0, 0), (0.5, 0.5, 0.5), (3.5, 4.0)),          # the two sides of a power of two: the exponents differ
    ((2, 9, 4), (0, 0, 8), (1.5, 1.5, 2.0), (255.25, 256.0)),     # ... in a bit of the select's top digit (bits 55..63 of the key)
])
def test_ranks_part_at_a_power_of_two(near, far, spacing, sq):
    """The issue names 3.75 and 4.0; 3.75 = 15 / 4 cannot be a squared distance on a grid with dyadic spacings (15 * 4^j is of the form
    4^j (8 b + 7): no sum of three squares), so the pair is 3.5 and 4.0, which straddles the same power of two.  The second pair parts in
    the top digit of the 11-bit select (exponent bit 3)."""
    gt, pred = sr.three_points(near, far)
    assert (float(sr.pass_order_square(near, spacing)), float(sr.pass_order_square(far, spacing))) == sq
    counts, values = _check(gt, pred, 2, spacing)
    assert (values[0][0], values[0][1]) == sq


def test_ranks_part_at_the_last_digit():
    """Two squared distances one ulp apart (non-dyadic spacing): the two ranks share every digit of the select but the last one."""
    near, far = (7, 0, 2), (1, 2, 4)
    lo, hi = sr.pass_order_square(near, sr.NON_DYADIC), sr.pass_order_square(far, sr.NON_DYADIC)
    assert np.nextafter(lo, np.inf) == hi      # precondition on the inputs, in the arithmetic the issue prescribes for the passes
    gt, pred = sr.three_points(near, far)
    counts, values = _check(gt, pred, 2, sr.NON_DYADIC)
    assert values[0][0] == lo and values[0][1] == hi


def test_four_classes_and_the_empty_mask_conventions():
    gt, pred = sr.four_class_maps()
    spacing = (1.5, 1.5, 2.0)
    _check(gt, pred, 5, spacing)
    recs = _surface_records_kernels(_t(gt), _t(pred), 5, spacing, 1.0)
    want = surface_metrics_multiclass(gt, pred, 5, spacing, 1.0)          # host arrays: the numpy path
    sr.check_dict(recs[0], sr.Reference(gt, pred, 1, spacing), spacing, 1.0)
    sr.check_dict(want[0], sr.Reference(gt, pred, 1, spacing), spacing, 1.0)
    one = {k: 373.128664 for k in recs[1]}
    one.update(dice=0, nsd=0.0)
    none = {k: 0 for k in recs[1]}
    none.update(dice=1, nsd=1.0)
    for got in (recs, want):
        assert got[1] == one and got[3] == one and got[2] == none
        for i in (1, 2, 3):
            assert [type(v) for v in got[i].values()] == [type(v) for v in (one if i != 2 else none).values()]
        assert isinstance(got[2]["dice"], int) and isinstance(got[2]["hd95"], int) and isinstance(got[2]["nsd"], float)
    pairs = _cal_metric_surface_kernels(_t(gt), _t(pred), 5, spacing)
    host = cal_metric_multiclass(gt, pred, 5, voxelspacing=spacing)
    assert pairs == host == [cal_metric(gt == c, pred == c, spacing) for c in range(1, 5)]
    assert [[type(v) for v in m] for m in pairs] == [[type(v) for v in m] for m in host]
    assert pairs[1] == (0, 373.128664) and pairs[2] == (1, 0) and isinstance(pairs[2][1], int)


def test_unit_spacing_pairs_equal_the_integer_path():
    gt, pred = sr.four_class_maps()
    assert _cal_metric_surface_kernels(_t(gt), _t(pred), 5, (1.0, 1.0, 1.0)) == _cal_metric_kernels(_t(gt), _t(pred), 5)


def test_two_calls_are_bit_equal():
    gt, pred = sr.ellipsoids(1)
    a = ops.seg_surface_metrics(_t(pred), _t(gt), 2, sr.NON_DYADIC, 2.0)
    b = ops.seg_surface_metrics(_t(pred), _t(gt), 2, sr.NON_DYADIC, 2.0)
    assert torch.equal(a[0], b[0]) and a[1].numpy().tobytes() == b[1].numpy().tobytes()


def test_label_dtypes():
    gt, pred = sr.ellipsoids(0, (9, 11, 8))
    want = _run(gt, pred, 2, (1.5, 1.5, 2.0))
    for gd, pd in ((np.uint8, np.uint8), (np.int64, np.int64), (np.bool_, np.int64), (np.int64, np.uint8)):
        assert _run(gt.astype(gd), pred.astype(pd), 2, (1.5, 1.5, 2.0)) == want


@pytest.mark.parametrize("spacing", [(0.0, 1.0, 1.0), (1.0, -1.0, 1.0), (1.0, 1.0, float("nan")), (1.0, 1.0), (1.0, float("inf"), 1.0)])
def test_bad_spacing_is_refused(spacing):
    a = torch.zeros((4, 4, 4), dtype=torch.int64)
    with pytest.raises(ValueError):
        ops.seg_surface_metrics(a, a, 2, spacing)


def test_bad_arguments_are_refused():
    a = torch.zeros((4, 4, 4), dtype=torch.int64)
    for tol in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ops.seg_surface_metrics(a, a, 2, (1, 1, 1), tol)
    for nc in (1, 257):
        with pytest.raises(ValueError):
            ops.seg_surface_metrics(a, a, nc, (1, 1, 1))
    with pytest.raises(ValueError):
        ops.seg_surface_metrics(a, torch.zeros((4, 4, 5), dtype=torch.int64), 2, (1, 1, 1))
    with pytest.raises(ValueError):
        ops.seg_surface_metrics(a[None], a[None], 2, (1, 1, 1))
    with pytest.raises(TypeError):
        ops.seg_surface_metrics(a.float(), a, 2, (1, 1, 1))
    # the C entry point itself: -1 with a message, nothing launched (the output buffers stay as they were)
    L = _lib.lib()
    counts = torch.full((1, 7), 77, dtype=torch.int64)
    values = torch.full((1, 6), 77.0, dtype=torch.float64)
    ws = torch.empty(L.icl_seg_surface_ws_bytes(4, 4, 4, 2), dtype=torch.uint8)
    bad = [dict(s0=0.0), dict(s1=-2.0), dict(s2=float("nan")), dict(s0=float("inf")), dict(tol=-0.5), dict(tol=float("nan")), dict(nc=1),
           dict(nc=257), dict(n0=0), dict(dtype=4)]
    for kw in bad:
        arg = dict(s0=1.0, s1=1.0, s2=1.0, tol=1.0, nc=2, n0=4, dtype=8)
        arg.update(kw)
        rc = L.icl_seg_surface_metrics(a.data_ptr(), arg["dtype"], a.data_ptr(), 8, arg["n0"], 4, 4, arg["nc"], arg["s0"], arg["s1"], arg["s2"],
                                       arg["tol"], counts.data_ptr(), values.data_ptr(), ws.data_ptr(), None)
        assert rc == -1 and b"seg_surface_metrics" in L.icl_last_error(), kw
        assert int(counts.min()) == 77 and float(values.min()) == 77.0
    assert L.icl_seg_surface_ws_bytes(4, 4, 4, 1) == -1 and L.icl_seg_surface_ws_bytes(4, 4, 4, 257) == -1


def test_host_tensor_is_refused_by_the_product_library():
    _lib._use_library_for_tests(None)
    try:
        a = torch.zeros((4, 4, 4), dtype=torch.int64)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.seg_surface_metrics(a, a, 2, (1.0, 1.0, 1.0))
    finally:
        _lib._use_library_for_tests(build_emu(), host_pointers=True)


# the sizes that the library of commit ca1119d2aa3a5921954c12ced9f9332573bd19a7 (the parent of the one that put the workspace carver into the
# launchers) returns, recorded from its emulation build: the layout of the workspace has not moved
@pytest.mark.parametrize("shape, nc, nbytes", [((1, 1, 1), 2, 141824), ((5, 7, 9), 3, 151808), ((3, 300, 2), 256, 848128), ((96, 96, 96), 16, 30258944)])
def test_workspace_size_is_that_of_the_earlier_layout(shape, nc, nbytes):
    assert _lib.lib().icl_seg_surface_ws_bytes(*shape, nc) == nbytes
