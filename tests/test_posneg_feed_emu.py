"""Foreground-balanced crops (RandCropByPosNegLabel feed: rank_count_kernel, rank_scan_kernel, rank_select_kernel in
csrc/kernels/rankindex.h, volume_feed_kernel<V, true> in datafeed.h, icl_rank_index_build / icl_rank_select / icl_volume_feed_origins,
icl_amd/dataloaders/amos.py) on the CPU emulation of the kernel sources, against the numpy restatement in tests/posneg_feed_ref.py; the
GPU run is in test_gpu_posneg_feed.py.  Every comparison is exact.  kRankTile = 1024, and the shapes are those of the reference module:
693 voxels (less than a tile), 1,024 (exactly one), 4,199 (four tiles and a partial one), a constructed 4,608-voxel volume with two whole
tiles of background between foreground voxels, and (5, 3, 2), smaller than the ROI on every axis.  Parity with MONAI's own code is
unpinned (MONAI is not installed)."""
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
import amos_feed_ref as aref  # noqa: E402
import posneg_feed_ref as ref  # noqa: E402

from icl_amd import _lib  # noqa: E402
from icl_amd.dataloaders.amos import (KIND_BG, KIND_FG, AMOSDeviceLoader, ForegroundIndex, OnDeviceAugmentPosNeg,  # noqa: E402
                                      draw_posneg_params)
from icl_amd.dataloaders.brats2019 import DeviceVolumeStore  # noqa: E402


@pytest.fixture(scope="module")
def emu_library():
    _lib._use_library_for_tests(build_emu(), host_pointers=True)
    yield
    _lib._use_library_for_tests(None)


@pytest.fixture(scope="module")
def store(emu_library):
    return ref.small_store("cpu")


@pytest.fixture(scope="module")
def index(store):
    return ForegroundIndex(store, ref.THRESHOLD)


def test_index_equals_numpys_per_tile_cumulative_counts(store):
    index = ref.check_index(store, [ref.volume(v) for v in range(len(ref.SHAPES))])
    gap = ref.SHAPES.index(ref.GAP_SHAPE)
    fg, bg = ref.index_arrays(index, gap)
    assert fg[1] == fg[2] == fg[3] and fg[0] < fg[1] and fg[3] < fg[4]      # two whole tiles without foreground, members around them
    assert bg[2] - bg[1] == ref.TILE and bg[3] == bg[4] and bg[4] < bg[5]    # a full tile | a tile without background | the partial tile


def test_index_of_an_empty_list_and_of_nan_voxels(emu_library):
    volumes = ref.special_volumes()
    index = ref.check_index(DeviceVolumeStore(volumes, "cpu"), volumes)
    assert index.n_fg[0] == 0 and index.n_bg[0] > 0            # all-zero label
    assert index.n_bg[1] == 0 and index.n_fg[1] > 0            # no background above the threshold
    assert index.n_bg[2] < index.n_bg[0]                       # NaN voxels are in neither list ...
    assert index.n_fg[2] == index.n_fg[1]                      # ... unless their label says foreground


def test_index_with_another_threshold(store):
    ref.check_index(store, [ref.volume(v) for v in range(len(ref.SHAPES))], threshold=0.5)


@pytest.mark.parametrize("roi", [ref.ROI_SCALAR, ref.ROI_QUAD])
@pytest.mark.parametrize("v", range(4))
def test_select_every_rank_of_both_lists(store, index, v, roi):
    """First and last rank, both sides of every tile boundary, the empty tiles in between: all of them."""
    n = ref.check_select_exhaustive(store, index, v, roi)
    assert n == index.n_fg[v] + index.n_bg[v] > 0


def test_select_partial_launches(store, index):
    ref.check_select_exhaustive(store, index, 0, ref.ROI_SCALAR, per_launch=5)


def test_select_with_a_roi_larger_than_the_volume_and_equal_to_it(store, index):
    small = ref.SHAPES.index((5, 3, 2))
    for roi in (ref.ROI_SCALAR, ref.ROI_QUAD):
        ref.check_select_exhaustive(store, index, small, roi)                 # s = n on every axis: the origin is 0
    ref.check_select_exhaustive(store, index, 0, ref.SHAPES[0])                # ROI = volume
    ref.check_select_exhaustive(store, index, 0, (3, 20, 4))                   # one axis larger than the volume's, the others inside


def test_unaligned_volumes_take_the_narrow_loads_and_give_the_same_index_and_origins(emu_library):
    vols = (2, 3)
    store = ref.misaligned_store("cpu", vols)
    index = ref.check_index(store, [ref.volume(v) for v in vols])
    for slot, v in enumerate(vols):
        ref.check_select_exhaustive(store, index, v, ref.ROI_QUAD, slot=slot)


@pytest.mark.parametrize("roi", [ref.ROI_SCALAR, ref.ROI_QUAD])
def test_batch_equals_the_forward_chain_on_the_references_crop(store, index, roi):
    """20 samples (two launches) on the one-voxel (6, 6, 5) and the four-voxel (6, 6, 8) path; out= with both label forms; runs repeat."""
    ref.check_end_to_end(store, index, roi)


def test_batch_draws_its_own_rows_and_feeds_the_loader(store, index):
    roi = ref.ROI_QUAD
    feed = OnDeviceAugmentPosNeg(store, index, roi, num_samples=3, rng=np.random.RandomState(3), flip_prob=0.5, rot_prob=0.5)
    state = feed.rng.get_state()
    rows = feed.draw([2, 0])
    feed.rng.set_state(state)
    assert len(rows) == 6 and [r[:3] for r in rows] == [ref.SHAPES[2]] * 3 + [ref.SHAPES[0]] * 3          # volume-major
    batches = list(AMOSDeviceLoader(feed, [(2, 0)]))
    assert len(batches) == 1 and batches[0]["image"].shape == (6, 1, *roi)
    want = [aref.forward_chain(*ref.volume(v), ref.feed_row(v, row, roi), roi) for v, row in zip([2, 2, 2, 0, 0, 0], rows)]
    assert ref.same(batches[0]["image"].numpy(), np.stack([w[0] for w in want]))
    assert ref.same(batches[0]["label"].numpy(), np.stack([w[1] for w in want]))


def test_draws_follow_the_documented_sequence():
    shape, roi = (13, 17, 19), (6, 6, 8)
    for seed, kw in ((1, {}), (2, dict(flip_prob=0.5, rot_prob=0.9, scale_factor=0.1, scale_prob=0.7, shift_prob=0.6)),
                     (3, dict(pos=3, neg=1, num_samples=7, rot_prob=1.0, max_k=2)), (4, dict(pos=0, neg=1)), (5, dict(pos=1, neg=0))):
        rec = ref.RecordingRNG(seed)
        rows = draw_posneg_params(shape, roi, 1400, 900, rec, **kw)
        want_rows, want_calls = ref.documented_draws(seed, shape, roi, 1400, 900, **kw)
        assert rows == want_rows and rec.calls == want_calls, (seed, kw)
        k = kw.get("num_samples", 4)
        assert len(rows) == k and all(len(r) == 18 and r[3:6] == (0, 0, 0) for r in rows)
        assert [c[0] for c in rec.calls[:2 * k]] == ["rand", "randint"] * k      # all centres first, then the tails
        assert all(0 <= r[17] < (1400 if r[16] == KIND_FG else 900) for r in rows)
        if "pos" in kw and kw["pos"] == 0:
            assert all(r[16] == KIND_BG for r in rows)
        if "neg" in kw and kw["neg"] == 0:
            assert all(r[16] == KIND_FG for r in rows)


def test_draws_with_an_empty_list():
    shape, roi = (7, 9, 11), (6, 6, 5)
    for n_fg, n_bg, kind in ((0, 50, KIND_BG), (40, 0, KIND_FG)):
        rec = ref.RecordingRNG(9)
        rows = draw_posneg_params(shape, roi, n_fg, n_bg, rec, pos=1, neg=1)
        want_rows, want_calls = ref.documented_draws(9, shape, roi, n_fg, n_bg)
        assert rows == want_rows and rec.calls == want_calls            # the draws are still made
        assert all(r[16] == kind for r in rows)
        assert [c for c in rec.calls[:8] if c[0] == "randint"] == [("randint", max(n_fg, n_bg))] * 4
    with pytest.raises(ValueError, match="No sampling location available"):
        draw_posneg_params(shape, roi, 0, 0, np.random.RandomState(0))
    with pytest.raises(ValueError, match="pos = -1"):
        draw_posneg_params(shape, roi, 5, 5, np.random.RandomState(0), pos=-1)
    with pytest.raises(ValueError, match="not both 0"):
        draw_posneg_params(shape, roi, 5, 5, np.random.RandomState(0), pos=0, neg=0)
    with pytest.raises(TypeError):
        draw_posneg_params(shape, roi, 5, 5, np.random.RandomState(0), flip_probability=0.5)


def test_batch_refuses_what_the_device_cannot_check(store, index):
    roi = ref.ROI_SCALAR
    feed = OnDeviceAugmentPosNeg(store, index, roi, num_samples=1)
    good = ref.make_row(ref.SHAPES[0], roi, KIND_FG, index.n_fg[0] - 1)
    feed.batch([0], params=[good])
    with pytest.raises(ValueError, match="rank .* outside the foreground list of volume 0"):
        feed.batch([0], params=[good[:17] + (index.n_fg[0],)])
    with pytest.raises(ValueError, match="outside the background list"):
        feed.batch([0], params=[good[:16] + (KIND_BG, index.n_bg[0])])
    with pytest.raises(ValueError, match="rank -1"):
        feed.batch([0], params=[good[:17] + (-1,)])
    with pytest.raises(ValueError, match="kind 2"):
        feed.batch([0], params=[good[:16] + (2, 0)])
    with pytest.raises(ValueError, match="1 parameter rows of 18 values"):
        feed.batch([0], params=[good[:16]])
    with pytest.raises(ValueError, match="volume 1 is"):
        feed.batch([1], params=[good])
    with pytest.raises(ValueError, match="not square"):
        OnDeviceAugmentPosNeg(store, index, (6, 5, 5))
    with pytest.raises(ValueError, match="odd quarter turn"):
        OnDeviceAugmentPosNeg(store, index, (6, 5, 5), num_samples=1, rot_prob=0).batch(
            [0], params=[ref.make_row(ref.SHAPES[0], (6, 5, 5), KIND_FG, 0, k=1)])
    with pytest.raises(ValueError, match="not built from this store"):
        OnDeviceAugmentPosNeg(ref.small_store("cpu"), index, roi)
    image = torch.zeros(2, 1, *roi)
    with pytest.raises(ValueError, match="out (image|label) must be"):
        OnDeviceAugmentPosNeg(store, index, roi, num_samples=2).batch([0], params=[good, good],
                                                                     out=(image, torch.zeros((2, 1, *roi), dtype=torch.int32)))
    # a volume without foreground and one without background: the draw goes to the other list; neither: an error at draw time
    volumes = ref.special_volumes()
    st = DeviceVolumeStore(volumes + [(-np.abs(np.nan_to_num(volumes[0][0])), volumes[0][1])], "cpu")
    special = OnDeviceAugmentPosNeg(st, ForegroundIndex(st), ref.ROI_QUAD, rng=np.random.RandomState(1))
    rows = special.draw([0, 1])
    assert [r[16] for r in rows] == [KIND_BG] * 4 + [KIND_FG] * 4
    assert special.batch([0, 1], params=rows)["image"].shape == (8, 1, *ref.ROI_QUAD)
    with pytest.raises(ValueError, match="No sampling location available"):
        special.batch([3])


def test_extents_monai_could_not_index_are_refused(emu_library):
    class Wide:                                                           # a stand-in volume: only its shape is looked at
        shape = (70000, 1, 1)

    class WideStore:
        device = torch.device("cpu")
        images, labels = [Wide()], [Wide()]

    with pytest.raises(ValueError, match="below 65,536"):
        ForegroundIndex(WideStore())


_KEEP = []


def test_select_launcher_refuses_bad_arguments_and_writes_nothing(store, index):
    roi = ref.ROI_SCALAR
    shape = ref.SHAPES[0]
    rc, origins = ref.raw_select(store, index, [(0, KIND_FG, 3)], roi)
    assert rc == 0 and origins.tolist() == [ref.origin_reference(shape, roi, ref.lists(*ref.volume(0))[0][3])]

    def refused(match, samples=None, **kw):
        rc, origins = ref.raw_select(store, index, samples or [(0, KIND_FG, 3)], roi, **kw)
        assert rc == -1
        with pytest.raises(RuntimeError, match=match):
            _lib.check(rc, "rank_select")
        assert (origins == -7).all()

    for null in range(6):
        refused("null pointer", null=null)
    refused("batch 0 out of range", batch=0)
    refused("batch 17 out of range", samples=[(0, KIND_FG, 3)] * 16, batch=17)
    refused("kind 2", samples=[(0, 2, 3)])
    refused("kind -1", samples=[(0, KIND_FG, 0), (0, -1, 3)])                      # the second sample: the first is not written either
    refused("rank -1", samples=[(0, KIND_BG, -1)])
    refused("crop size 0 of axis 1 outside 1..9", samples=[(0, KIND_FG, 3, (6, 0, 5))])
    refused("crop size 12 of axis 2 outside 1..11", samples=[(0, KIND_FG, 3, (6, 6, 12))])
    refused("each must be in 1..65535", samples=[(0, KIND_FG, 3, None, (7, 0, 11))])
    refused("each must be in 1..65535", samples=[(0, KIND_FG, 3, None, (65536, 9, 11))])
    refused("more than 2\\^31 - 1 voxels", samples=[(0, KIND_FG, 3, None, (2048, 2048, 512))])


def raw_build(image, label, shape, null=None):
    fg = torch.full((8,), -7, dtype=torch.int32)
    bg = torch.full((8,), -7, dtype=torch.int32)
    args = [image.data_ptr(), label.data_ptr(), *shape, ctypes.c_float(0.0), fg.data_ptr(), bg.data_ptr()]
    if null is not None:
        args[null] = None
    return _lib.lib().icl_rank_index_build(*args, None), fg, bg


def test_build_launcher_refuses_bad_arguments_and_writes_nothing(store):
    image, label = store.images[0], store.labels[0]
    rc, fg, bg = raw_build(image, label, ref.SHAPES[0])
    assert rc == 0 and fg[0] == 0 and bg[0] == 0 and fg[1] + bg[1] > 0 and (fg[2:] == -7).all()      # 693 voxels: one tile, two entries
    for kw in (dict(null=0), dict(null=1), dict(null=6), dict(null=7)):
        rc, fg, bg = raw_build(image, label, ref.SHAPES[0], **kw)
        assert rc == -1 and b"null pointer" in _lib.lib().icl_last_error() and (fg == -7).all() and (bg == -7).all()
    for shape, text in (((0, 9, 11), b"1..65535"), ((7, 9, 65536), b"1..65535"), ((65535, 65535, 1), b"2^31 - 1 voxels")):
        rc, fg, bg = raw_build(image, label, shape)
        assert rc == -1 and text in _lib.lib().icl_last_error() and (fg == -7).all() and (bg == -7).all()


def raw_feed(store, index, roi, rows, vols, batch=None, null=None, origin=(0, 0, 0)):
    """icl_volume_feed_origins through ctypes with sentinel-filled outputs and the given origin for every sample."""
    m = len(rows)
    ptrs = ctypes.c_void_p * m
    origins = torch.tensor([origin] * m, dtype=torch.int32)
    args = [ptrs(*[store.images[i].data_ptr() for i in vols]), ptrs(*[store.labels[i].data_ptr() for i in vols]),
            (ctypes.c_int32 * (14 * m))(*[int(v) for r in rows for v in r[:14]]), (ctypes.c_float * (2 * m))(*[float(v) for r in rows for v in r[14:16]]),
            m if batch is None else batch, origins.data_ptr()]
    image = torch.full((m, 1, *roi), -7.0)
    label = torch.full((m, *roi), -7, dtype=torch.int64)
    outs = [image.data_ptr(), label.data_ptr()]
    _KEEP.append((args, origins))
    if null is not None:
        if null < 6:
            args[null] = None
        else:
            outs[null - 6] = None
    return _lib.lib().icl_volume_feed_origins(*args, *outs, *roi, None), image, label


def test_feed_launcher_refuses_bad_arguments_and_writes_nothing(store, index):
    roi = ref.ROI_SCALAR
    shape = ref.SHAPES[0]
    good = ref.make_row(shape, roi, KIND_FG, 0, flip=3, k=1, add=0.0625)
    rc, image, label = raw_feed(store, index, roi, [good], [0], origin=(1, 3, 6))
    assert rc == 0 and not (image == -7).any() and not (label == -7).any()
    want = aref.forward_chain(*ref.volume(0), (*good[:3], 1, 3, 6, *good[6:16]), roi)
    assert ref.same(image.numpy()[0], want[0]) and ref.same(label.numpy(), want[1])
    # an origin outside [0, n - s] cannot come from the select kernel; the gather clamps it instead of reading outside the volume
    for origin, clamped in (((-5, 99, 7), (0, 3, 6)), ((2, -1, -1), (1, 0, 0))):
        rc, image, label = raw_feed(store, index, roi, [good], [0], origin=origin)
        want = aref.forward_chain(*ref.volume(0), (*good[:3], *clamped, *good[6:16]), roi)
        assert rc == 0 and ref.same(image.numpy()[0], want[0]) and ref.same(label.numpy(), want[1])

    def edit(pos, value):
        return good[:pos] + (value,) + good[pos + 1:]

    def refused(match, rows=None, roi_=roi, **kw):
        rc, image, label = raw_feed(store, index, roi_, rows or [good], [0] * len(rows or [good]), **kw)
        assert rc == -1
        with pytest.raises(RuntimeError, match=match):
            _lib.check(rc, "volume_feed_origins")
        assert (image == -7).all() and (label == -7).all()

    for null in (0, 1, 2, 3, 5, 6, 7):
        refused("volume_feed_origins: null pointer", null=null)
    refused("batch 0 out of range", batch=0)
    refused("batch 17 out of range", rows=[good] * 16, batch=17)
    assert raw_feed(store, index, roi, [edit(3, -1), edit(5, 99)], [0, 0])[0] == 0      # the rows' origin fields are not read
    refused("crop size 0 of axis 1 outside 1..9", rows=[edit(7, 0)])
    refused("crop size 12 of axis 2 outside 1..11", rows=[edit(8, 12)])
    refused("left pad -1", rows=[edit(9, -1)])
    refused("left pad 1 \\+ crop size 5 of axis 2 outside the output extent 5", rows=[edit(11, 1)])
    refused("flip mask 8", rows=[edit(12, 8)])
    refused("k = 4 outside 0..3", rows=[edit(13, 4)])
    roi_ns = (6, 5, 5)
    even = ref.make_row(shape, roi_ns, KIND_FG, 0, k=2)
    odd = ref.make_row(shape, roi_ns, KIND_FG, 0, k=3)
    assert raw_feed(store, index, roi_ns, [even], [0])[0] == 0
    refused("an odd rot90 needs R0 == R1", rows=[even, odd], roi_=roi_ns)


def test_the_feed_with_host_origins_is_unchanged(emu_library):
    """icl_volume_feed shares its body and its checks with the new entry: one sweep of the AMOS feed's own reference still passes."""
    assert aref.check_sweep(aref.small_store("cpu"), aref.ROI_QUAD) == 288
