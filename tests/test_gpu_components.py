"""Connected components and the keep-largest filter on the MI355X (kernels/components.h): ops.seg_components / seg_filter_components,
val_3D.keep_components and the ``postprocess=`` keyword of the validation loops against scipy.ndimage.label.  Cases and reference:
tests/components_ref.py (the same cases run on the CPU emulator in test_components_emu.py).  Every instantiation is launched: the
tile and merge kernels for uint8 and int64 maps under each connectivity, the reduce and filter kernels for both element sizes."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import components_ref as cr  # noqa: E402

from icl_amd import ops, val_2D, val_3D  # noqa: E402
from icl_amd.utils.hashfill import synthetic_segmentation  # noqa: E402
from icl_amd.val_3D import keep_components  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from icl_amd import _lib
    assert _lib.lib_path().endswith("libicl_hip.so"), "GPU tests must run on the HIP library"
    return torch.device("cuda", 0)


def _up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _check_labels(m, nc, k, dev):
    labels, counts = ops.seg_components(_up(m, dev), nc, k)
    assert labels.is_cuda and counts.is_cuda and labels.dtype == torch.int32 and counts.dtype == torch.int64
    cr.check_labels(m, labels.cpu().numpy(), counts.cpu().numpy(), nc, k)


@pytest.mark.parametrize("k", cr.CONNECTIVITIES)
@pytest.mark.parametrize("name", list(cr.CASES))
def test_case(dev, name, k):
    m, nc = cr.CASES[name]()
    _check_labels(m, nc, k, dev)
    t = _up(m, dev)
    for keep_largest, min_size in cr.filter_settings(m, nc, k):
        out = ops.seg_filter_components(t, nc, k, keep_largest, min_size)
        assert out.is_cuda and out.dtype == t.dtype
        cr.check_filter(m, out.cpu().numpy(), nc, k, keep_largest, min_size)


@pytest.mark.parametrize("k", cr.CONNECTIVITIES)
@pytest.mark.parametrize("dtype", [np.uint8, np.int64])
def test_scattered_prediction_64x80x72(dev, dtype, k):
    """An early-training prediction with 16 classes: thousands of specks, hundreds of tiles, more workgroups in the reduction than it
    keeps partials."""
    _, pred = synthetic_segmentation((64, 80, 72), 16, 5, scatter=0.05)
    m = pred.astype(dtype)
    _check_labels(m, 16, k, dev)
    out = ops.seg_filter_components(_up(m, dev), 16, k)
    cr.check_filter(m, out.cpu().numpy(), 16, k)


def test_more_voxels_than_one_grid_pass(dev):
    """128 x 128 x 130 voxels are more than the 8192 x 256 threads of the merge, flatten and filter grids: every thread takes a second
    voxel.  One big ragged blob and scattered specks."""
    _, pred = synthetic_segmentation((128, 128, 130), 2, 9, scatter=0.02)
    m = pred.astype(np.uint8)
    _check_labels(m, 2, 1, dev)
    out = ops.seg_filter_components(_up(m, dev), 2, 1)
    cr.check_filter(m, out.cpu().numpy(), 2, 1)


@pytest.mark.parametrize("k", cr.CONNECTIVITIES)
def test_ties_keep_the_first(dev, k):
    for axis in range(3):
        m, nc = cr.ties(axis)
        assert ops.seg_filter_components(_up(m, dev), nc, k).cpu().numpy().ravel().tolist() == [1, 1, 0, 0, 0]


@pytest.mark.parametrize("dtype", [np.uint8, np.int64])
def test_out_may_be_the_map(dev, dtype):
    m, nc = cr.CASES["random_nc4_d5"]()
    m = m.astype(dtype)
    t = _up(m, dev)
    assert ops.seg_filter_components(t, nc, 2, True, 0, out=t) is t
    cr.check_filter(m, t.cpu().numpy(), nc, 2, True, 0)


@pytest.mark.parametrize("k", cr.CONNECTIVITIES)
def test_two_runs_are_bit_equal(dev, k):
    for name in ("serpentine", "one_class", "random_nc17_d8"):
        m, nc = cr.CASES[name]()
        t = _up(m, dev)
        a, b = ops.seg_components(t, nc, k), ops.seg_components(t, nc, k)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert torch.equal(ops.seg_filter_components(t, nc, k), ops.seg_filter_components(t, nc, k))


def test_bad_arguments_are_refused(dev):
    a = torch.zeros((4, 4, 4), dtype=torch.int64, device=dev)
    for fn in (ops.seg_components, ops.seg_filter_components):
        for nc in (1, 257):
            with pytest.raises(ValueError):
                fn(a, nc)
        for k in (0, 4):
            with pytest.raises(ValueError):
                fn(a, 2, k)
        with pytest.raises(TypeError):
            fn(a.float(), 2)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(a.cpu(), 2)
    with pytest.raises(ValueError):
        ops.seg_filter_components(a, 2, 1, True, -1)


def _forbidden(*args, **kwargs):
    raise AssertionError("the device run filtered a map on the host")


@pytest.mark.parametrize("k", cr.CONNECTIVITIES)
@pytest.mark.parametrize("name", ["serpentine", "corner_and_edge", "out_of_range_int64", "bool_map", "leading_axis", "random_nc17_d5"])
def test_keep_components_device_equals_host(dev, monkeypatch, name, k):
    m, nc = cr.CASES[name]()
    t = _up(m, dev)
    for keep_largest, min_size in cr.filter_settings(m, nc, k)[:4]:
        monkeypatch.setenv("ICL_VAL_COMPONENTS", "device")
        with monkeypatch.context() as mp:
            mp.setattr(val_3D, "_keep_components_host", _forbidden)
            got = keep_components(t, nc, k, keep_largest, min_size)
        monkeypatch.setenv("ICL_VAL_COMPONENTS", "host")
        want = keep_components(t, nc, k, keep_largest, min_size)
        for r in (got, want):      # still a device tensor of the input's dtype and shape
            assert torch.is_tensor(r) and r.device == t.device and r.dtype == t.dtype and r.shape == t.shape
        assert torch.equal(got, want)
        assert np.array_equal(got.cpu().numpy(), keep_components(m, nc, k, keep_largest, min_size))      # host data: scipy


class _RoundNet(torch.nn.Module):
    """logits[:, k] = -(x - k)^2: the arg-max is the input rounded to the nearest class — the prediction is the image."""

    def __init__(self, classes, dev):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1, device=dev))
        self.classes = classes

    def forward(self, x, inference=False):
        return torch.cat([-(x - k) ** 2 for k in range(self.classes)], dim=1)


def _loop_both_ways(monkeypatch, run):
    """run(postprocess=...) with the filter on the device (the host restatement made to fail if called), with ICL_VAL_COMPONENTS=host, and
    without the filter."""
    seen = []
    real = val_3D.keep_components

    def spy(label_map, *a, **kw):
        out = real(label_map, *a, **kw)
        seen.append((label_map, out))
        return out

    monkeypatch.setenv("ICL_VAL_COMPONENTS", "device")
    with monkeypatch.context() as mp:
        mp.setattr(val_3D, "_keep_components_host", _forbidden)
        mp.setattr(val_3D, "keep_components", spy)
        mp.setattr(val_2D, "keep_components", spy)
        got = run(postprocess="largest")
    assert seen
    for before, after in seen:      # the prediction went in and came out as a device tensor of one dtype
        assert torch.is_tensor(after) and after.is_cuda and after.dtype == before.dtype == torch.int64 and after.shape == before.shape
    monkeypatch.setenv("ICL_VAL_COMPONENTS", "host")
    want = run(postprocess="largest")
    monkeypatch.setenv("ICL_VAL_COMPONENTS", "device")
    plain = run(postprocess=None)
    assert plain == run()
    return got, want, plain


def test_all_case_base_postprocess_device_equals_host(dev, monkeypatch):
    net = _RoundNet(3, dev)
    cases = []
    for s in (0, 1):
        gt, pred = synthetic_segmentation((40, 48, 40), 3, 10 + s, scatter=0.02)
        cases.append((pred.astype(np.float32), gt))
    run = lambda **kw: val_3D.test_all_case_base(net, "unet_3D", None, num_classes=3, patch_size=(32, 48, 32), stride_xy=8, stride_z=8,  # noqa: E731
                                                 cases=list(cases), **kw)
    got, want, plain = _loop_both_ways(monkeypatch, run)
    assert got == want != plain and len(got) == 2 and all(len(m) == 2 for m in got)


def test_all_case_amos_postprocess_device_equals_host(dev, monkeypatch):
    net = _RoundNet(4, dev)
    gt, pred = synthetic_segmentation((50, 48, 44), 4, 30, scatter=0.02)      # narrower than the 96^3 window: padded, then cropped
    loader = [{"image": torch.from_numpy(pred.astype(np.float32)).view(1, 1, 50, 48, 44),
               "label": torch.from_numpy(gt.astype(np.int64)).view(1, 1, 50, 48, 44)}]
    run = lambda **kw: val_3D.test_all_case_amos(net, "unet_3D", loader, num_classes=4, **kw)      # noqa: E731
    got, want, plain = _loop_both_ways(monkeypatch, run)
    assert got == want != plain and len(got) == 3


@pytest.mark.parametrize("fn", ["test_single_volume", "test_single_volume_ours"])
def test_single_volume_postprocess_device_equals_host(dev, monkeypatch, fn):
    net = _RoundNet(4, dev)
    gt, pred = synthetic_segmentation((6, 80, 72), 4, 40, scatter=0.02)
    image = torch.from_numpy(pred.astype(np.float32)).unsqueeze(0)
    label = torch.from_numpy(gt).unsqueeze(0)
    run = lambda **kw: getattr(val_2D, fn)(image, label, net, classes=4, patch_size=(80, 72), **kw)      # noqa: E731
    got, want, plain = _loop_both_ways(monkeypatch, run)
    assert got == want != plain and len(got) == 3
