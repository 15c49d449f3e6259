"""Foreground-balanced crops on the MI355X, through the C ABI (rank_count_kernel, rank_scan_kernel, rank_select_kernel in
csrc/kernels/rankindex.h, volume_feed_kernel<V, true> in datafeed.h, icl_amd/dataloaders/amos.py): exactly the numpy restatement of
tests/posneg_feed_ref.py at the small shapes of test_posneg_feed_emu.py, one batch of 2 volumes x 4 samples at the trainer's 96^3 with
sparse labels, and one loader batch through the 16-class model."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import amos_feed_ref as aref  # noqa: E402
import posneg_feed_ref as ref  # noqa: E402

from icl_amd.dataloaders.amos import AMOSDeviceLoader, ForegroundIndex, OnDeviceAugmentPosNeg, amos_volume_store  # noqa: E402
from icl_amd.dataloaders.brats2019 import DeviceVolumeStore, TwoStreamBatchSampler  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from icl_amd import _lib
    assert _lib.lib_path().endswith("libicl_hip.so"), "GPU tests must run on the HIP library"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def store(dev):
    return ref.small_store(dev)


@pytest.fixture(scope="module")
def index(store):
    return ForegroundIndex(store, ref.THRESHOLD)


@pytest.fixture(scope="module")
def big(dev):
    st = amos_volume_store([ref.big_volume(j) for j in range(2)], dev)
    return st, ForegroundIndex(st, ref.THRESHOLD)


def test_index_on_the_gpu(store, dev):
    assert store.images[0].is_cuda
    ref.check_index(store, [ref.volume(v) for v in range(len(ref.SHAPES))])
    ref.check_index(store, [ref.volume(v) for v in range(len(ref.SHAPES))], threshold=0.5)
    volumes = ref.special_volumes()                       # an all-zero label, no background, NaN voxels
    special = ref.check_index(DeviceVolumeStore(volumes, dev), volumes)
    assert special.n_fg[0] == 0 and special.n_bg[1] == 0 and special.n_bg[2] < special.n_bg[0]


@pytest.mark.parametrize("roi", [ref.ROI_SCALAR, ref.ROI_QUAD])
def test_select_every_rank_of_both_lists_on_the_gpu(store, index, roi):
    for v in range(len(ref.SHAPES)):
        assert ref.check_select_exhaustive(store, index, v, roi) == index.n_fg[v] + index.n_bg[v]


def test_select_with_a_roi_equal_to_the_volume_and_partial_launches(store, index):
    ref.check_select_exhaustive(store, index, 0, ref.SHAPES[0])
    ref.check_select_exhaustive(store, index, 0, (3, 20, 4), per_launch=5)


def test_unaligned_volumes_on_the_gpu(dev):
    """Image 4 bytes past a 16-byte boundary, label 1 byte past a 4-byte boundary: the narrow loads, the same index and origins."""
    vols = (2, 3)
    st = ref.misaligned_store(dev, vols)
    ix = ref.check_index(st, [ref.volume(v) for v in vols])
    for slot, v in enumerate(vols):
        ref.check_select_exhaustive(st, ix, v, ref.ROI_QUAD, slot=slot)


@pytest.mark.parametrize("roi", [ref.ROI_SCALAR, ref.ROI_QUAD])
def test_batch_equals_the_forward_chain_on_the_gpu(store, index, roi):
    ref.check_end_to_end(store, index, roi)


def test_eight_samples_at_the_trainers_roi_with_sparse_labels(big):
    """(130, 101, 70) and (60, 200, 111) with five small balls of labels each -> 2 x 4 crops of 96^3; two runs bit-equal."""
    st, ix = big
    indices, rows, want_image, want_label = ref.big_batch()
    for j in range(2):
        want = ref.index_reference(*ref.big_volume(j))
        got = ref.index_arrays(ix, j)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    feed = OnDeviceAugmentPosNeg(st, ix, aref.BIG_ROI, num_samples=4)
    got = feed.batch(indices, params=rows)
    assert got["image"].shape == (8, 1, 96, 96, 96) and got["label"].shape == (8, 1, 96, 96, 96)
    gi, gl = got["image"].cpu().numpy(), got["label"].cpu().numpy()
    for j in range(8):
        assert ref.same(gi[j], want_image[j]), j
        assert ref.same(gl[j], want_label[j]), j
    assert all(int((gl[j] != 0).sum()) > 0 for j in (0, 1, 3, 4, 5, 7))          # a crop around a foreground voxel shows foreground
    again = feed.batch(indices, params=rows)
    assert ref.same_bits(got["image"], again["image"]) and torch.equal(got["label"], again["label"])


def test_a_posneg_loader_batch_feeds_the_16_class_model(big):
    """The trainer's loop head on one AMOSDeviceLoader batch of an OnDeviceAugmentPosNeg (2 indices x 2 samples): `model(volume[:2],
    volume[2:])` of unet_3D_icl with 16 classes in training mode returns finite logits, and the label passes the trainer's expressions."""
    from icl_amd.networks.net_factory_3d import net_factory_3d
    from icl_amd.utils.hashfill import fill_like_reference_init
    st, ix = big
    labeled_bs = 2
    np.random.seed(1337)
    feed = OnDeviceAugmentPosNeg(st, ix, (96, 96, 96), num_samples=2)
    train_loader = AMOSDeviceLoader(feed, TwoStreamBatchSampler([0], [1], 2, 1))
    assert len(train_loader) == 1
    model = net_factory_3d(net_type="unet_3D_icl", in_chns=1, class_num=16)
    fill_like_reference_init(list(model.named_parameters()))
    model.train()
    seen = 0
    for i_batch, sampled_batch in enumerate(train_loader):
        volume_batch, label_batch = sampled_batch['image'], sampled_batch['label']
        volume_batch, label_batch = volume_batch.cuda(), label_batch.cuda()
        assert volume_batch.data_ptr() == sampled_batch['image'].data_ptr()
        assert volume_batch.shape == (4, 1, 96, 96, 96) and label_batch.shape == (4, 1, 96, 96, 96) and label_batch.dtype == torch.int64
        outputs = model(volume_batch[:labeled_bs], volume_batch[labeled_bs:])
        assert outputs[0].shape == (2, 16, 96, 96, 96) and bool(torch.isfinite(outputs[0]).all())
        target = label_batch[:labeled_bs].squeeze(1).long()
        assert target.shape == (2, 96, 96, 96) and 0 <= int(target.min()) and int(target.max()) <= 15
        assert torch.nn.functional.cross_entropy(outputs[0], target).isfinite()
        seen += 1
    assert seen == 1
