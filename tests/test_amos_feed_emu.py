"""AMOS data feed (volume_feed_kernel in csrc/kernels/datafeed.h, icl_volume_feed, icl_amd/dataloaders/amos.py) on the CPU emulation of
the kernel sources, against the numpy restatement of the forward chain in tests/amos_feed_ref.py; the GPU run is in
test_gpu_amos_feed.py.  Every comparison is exact.  Parity with MONAI's own code is unpinned (MONAI is not installed)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "hipemu"))
from build_emu import build_emu  # noqa: E402
import amos_feed_ref as ref  # noqa: E402

from icl_amd import _lib  # noqa: E402
from icl_amd.dataloaders.amos import OnDeviceAugmentAMOS  # noqa: E402


@pytest.fixture(scope="module")
def emu_library():
    _lib._use_library_for_tests(build_emu(), host_pointers=True)
    yield
    _lib._use_library_for_tests(None)


@pytest.fixture(scope="module")
def store(emu_library):
    return ref.small_store("cpu")


def test_scalar_path_sweep_equals_the_forward_chain(store):
    """ROI (6, 6, 5): 3 sources x 8 flip masks x 4 rotations x 3 intensity settings in launches of 16 mixed samples."""
    assert ref.check_sweep(store, ref.ROI_SCALAR) == 3 * 8 * 4 * 3


def test_quad_path_sweep_equals_the_forward_chain(store):
    """ROI (6, 6, 8): R2 % 4 == 0 and aligned outputs, one thread per four depth voxels, flip bit 2 among the masks."""
    assert ref.check_sweep(store, ref.ROI_QUAD) == 3 * 8 * 4 * 3
    assert ref.check_sweep(store, ref.ROI_QUAD, per_launch=5) == 288        # partial launches, other mixes


def test_misaligned_image_output_falls_back_and_is_still_equal(store):
    """ROI (6, 6, 8) with the image tensor 4 bytes past a 16-byte boundary: no 16-byte stores possible, same result."""
    ref.check_sweep(store, ref.ROI_QUAD, misaligned_image=True)


@pytest.mark.parametrize("roi", [ref.ROI_SCALAR, ref.ROI_QUAD])
def test_padded_voxels_hold_the_shift_and_label_zero(store, roi):
    ref.check_padded_voxels(store, roi)


@pytest.mark.parametrize("roi", [ref.ROI_SCALAR, ref.ROI_QUAD])
def test_inexact_products_are_rounded_twice_on_every_route(emu_library, roi):
    """mul = 1.1, add = 0.07 on hash-filled volumes: plain, device-origin and mixed affine launches (the emulator never contracts; the
    GPU run of the same check is the one that can fail)."""
    ref.check_twice_rounded_intensity("cpu", roi)


def test_out_tensors_are_filled_and_returned_as_views(store):
    roi = ref.ROI_QUAD
    indices, rows, want_image, want_label = ref.sweep(roi)
    feed = OnDeviceAugmentAMOS(store, roi)
    image = torch.full((3, 1, *roi), float("nan"))
    for label in (torch.full((3, 1, *roi), -1, dtype=torch.int64), torch.full((3, *roi), -1, dtype=torch.int64)):
        got = feed.batch(indices[:3], params=rows[:3], out=(image, label))
        assert got["image"].data_ptr() == image.data_ptr() and got["label"].data_ptr() == label.data_ptr()
        assert got["image"].shape == (3, 1, *roi) and got["label"].shape == (3, 1, *roi)
        assert np.array_equal(image.numpy(), want_image[:3]) and np.array_equal(label.numpy().reshape(3, 1, *roi), want_label[:3])
    good_label = torch.zeros((3, 1, *roi), dtype=torch.int64)
    for bad in ((torch.zeros(3, 1, *roi, dtype=torch.float64), good_label),            # dtype
                (torch.zeros(2, 1, *roi), good_label),                                 # shape
                (image, torch.zeros((3, 1, *roi), dtype=torch.int32)),                 # label dtype
                (torch.zeros(3, 1, roi[0], roi[2], roi[1]).transpose(3, 4), good_label),   # not contiguous
                (image.to("meta"), good_label)):                                       # device
        with pytest.raises(ValueError, match="out (image|label) must be"):
            feed.batch(indices[:3], params=rows[:3], out=bad)


_KEEP = []


def raw_call(store, roi, rows, indices, batch=None, null=None):
    """icl_volume_feed through ctypes with sentinel-filled outputs; returns (rc, image, label)."""
    m = len(rows)
    ptrs = ctypes.c_void_p * m
    args = [ptrs(*[store.images[i].data_ptr() for i in indices]), ptrs(*[store.labels[i].data_ptr() for i in indices]),
            (ctypes.c_int32 * (14 * m))(*[int(v) for r in rows for v in r[:14]]), (ctypes.c_float * (2 * m))(*[float(v) for r in rows for v in r[14:]])]
    image = torch.full((m, 1, *roi), -7.0)
    label = torch.full((m, *roi), -7, dtype=torch.int64)
    outs = [image.data_ptr(), label.data_ptr()]
    _KEEP.append((args, image, label))
    if null is not None:
        if null < 4:
            args[null] = None
        else:
            outs[null - 4] = None
    rc = _lib.lib().icl_volume_feed(*args, m if batch is None else batch, *outs, *roi, None)
    return rc, image, label


def test_launcher_refuses_bad_arguments_and_writes_nothing(store):
    roi = ref.ROI_SCALAR
    shape = ref.SOURCES[0]
    good = ref.make_row(shape, roi, (1, 0, 2), 3, 1, 1.0, 0.0625)
    rc, image, label = raw_call(store, roi, [good], [0])
    assert rc == 0 and not (image == -7).any() and not (label == -7).any()

    def edit(pos, value):
        return good[:pos] + (value,) + good[pos + 1:]

    def refused(match, rows=None, roi_=roi, **kw):
        rc, image, label = raw_call(store, roi_, rows or [good], [0] * len(rows or [good]), **kw)
        assert rc == -1
        with pytest.raises(RuntimeError, match=match):
            _lib.check(rc, "volume_feed")
        assert (image == -7).all() and (label == -7).all()

    for null in range(6):
        refused("null pointer", null=null)
    refused("batch 0 out of range", batch=0)
    refused("batch 17 out of range", rows=[good] * 16, batch=17)
    refused("crop \\[-1, ", rows=[edit(3, -1)])                          # c < 0
    refused("crop \\[0, 0 \\+ 0\\)", rows=[edit(7, 0)])                   # s < 1 (axis 1)
    refused("axis 2 outside the extent 8", rows=[edit(5, 4)])            # c + s > n: 4 + 5 > 8
    refused("left pad -1", rows=[edit(9, -1)])                           # l < 0
    refused("left pad 1 \\+ crop size 5 of axis 2 outside the output extent 5", rows=[edit(11, 1)])     # l + s > R
    refused("k = 4 outside 0..3", rows=[edit(13, 4)])
    refused("k = -1 outside 0..3", rows=[edit(13, -1)])
    # an odd k with R0 != R1: the second sample of the launch, so the first is not written either
    roi_ns = (6, 5, 5)
    even = ref.make_row(shape, roi_ns, (0, 0, 0), 0, 2)
    odd = ref.make_row(shape, roi_ns, (0, 0, 0), 0, 3)
    assert raw_call(store, roi_ns, [even], [0])[0] == 0
    refused("an odd rot90 needs R0 == R1", rows=[even, odd], roi_=roi_ns)
    with pytest.raises(RuntimeError, match="volume_feed failed"):
        _lib.check(raw_call(store, roi, [edit(13, 4)], [0])[0], "volume_feed")
