"""Affine stage of the 3-D feed on the MI355X, through the C ABI (volume_feed_affine_kernel in csrc/kernels/datafeed.h,
icl_volume_feed_affine / icl_volume_feed_affine_origins, icl_amd/dataloaders/amos.py): bit-equal to the numpy restatement of DESIGN.md §2
"Affine stage of the 3-D feed" (tests/affine_feed_ref.py) on the cases of test_affine_feed_emu.py and at the trainer's 96^3, and one
loader batch with the stage through the 16-class model."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import amos_feed_ref as aref  # noqa: E402
import affine_feed_ref as ref  # noqa: E402

from icl_amd.dataloaders.amos import AMOSDeviceLoader, OnDeviceAugmentAMOS, amos_volume_store  # noqa: E402
from icl_amd.dataloaders.brats2019 import TwoStreamBatchSampler  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from icl_amd import _lib
    assert _lib.lib_path().endswith("libicl_hip.so"), "GPU tests must run on the HIP library"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def small_store(dev):
    return aref.small_store(dev)


@pytest.fixture(scope="module")
def cube_store(dev):
    return ref.cube_store(dev)


@pytest.fixture(scope="module")
def random_store(dev):
    return ref.random_store(dev)


@pytest.fixture(scope="module")
def big_store(dev):
    volumes, _ = aref.big_batch()
    return amos_volume_store(volumes, dev)


@pytest.mark.parametrize("roi", [ref.ROI_SCALAR, ref.ROI_QUAD])
def test_identity_equals_the_plain_feed_on_the_gpu(small_store, roi):
    assert small_store.images[0].is_cuda
    assert ref.check_identity(small_store, roi) == 288


def test_proper_signed_permutations_on_the_gpu(cube_store):
    ref.check_signed_permutations(cube_store)


def test_dyadic_zooms_on_the_gpu(cube_store):
    ref.check_dyadic_zooms(cube_store)


@pytest.mark.parametrize("roi", ref.RANDOM_ROIS)
def test_random_matrices_equal_the_restatement_on_both_kernels(random_store, roi):
    assert ref.check_random(random_store, roi) == 24


@pytest.mark.parametrize("roi", ref.ROIS)
def test_nonfinite_voxels_count_only_where_a_tap_is_inside(dev, roi):
    assert ref.check_nonfinite(ref.nonfinite_store(dev), roi) == 24


def test_mixed_batch_of_17_is_two_launches_and_repeats_bit_for_bit(random_store):
    ref.check_mixed_batch(random_store)


def test_device_origins_equal_host_origins_and_are_clamped(dev):
    ref.check_device_origins(dev)


def test_refusals_write_nothing(small_store):
    ref.check_refusals(small_store)


def test_batch_of_four_at_the_trainers_roi_equals_the_restatement(big_store):
    """(130, 101, 70), (96, 96, 96), (97, 140, 96), (60, 200, 111) -> 96^3, every sample with a random M (+-0.5 rad, zoom 0.7 .. 1.4),
    every flip bit, every k, non-zero shifts."""
    cases = ref.big_cases()
    want_image, want_label = ref.reference(cases, "big", aref.BIG_ROI)
    got = OnDeviceAugmentAMOS(big_store, aref.BIG_ROI).batch([0, 1, 2, 3], params=[(*row, *M) for _, row, M in cases])
    assert got["image"].shape == (4, 1, 96, 96, 96) and got["label"].shape == (4, 1, 96, 96, 96)
    gi, gl = got["image"].cpu().numpy(), got["label"].cpu().numpy()
    for j in range(4):
        assert np.array_equal(gi[j], want_image[j]), j
        assert np.array_equal(gl[j], want_label[j]), j


def test_a_loader_batch_with_the_affine_stage_feeds_the_16_class_model(big_store):
    """The AMOS trainer's loop head (:216-227) on one AMOSDeviceLoader batch whose four samples all drew an affine."""
    from icl_amd.networks.net_factory_3d import net_factory_3d
    from icl_amd.utils.hashfill import fill_like_reference_init
    labeled_bs = 2
    feed = OnDeviceAugmentAMOS(big_store, (96, 96, 96), rng=np.random.RandomState(1337), affine_prob=1.0, rotate_range=0.5, zoom_range=(0.7, 1.4))
    state = feed.rng.get_state()
    assert all(len(row) == 25 for row in feed.draw([0, 2, 1, 3]))
    feed.rng.set_state(state)
    train_loader = AMOSDeviceLoader(feed, TwoStreamBatchSampler([0, 1], [2, 3], 4, 2))
    assert len(train_loader) == 1
    model = net_factory_3d(net_type="unet_3D_icl", in_chns=1, class_num=16)
    fill_like_reference_init(list(model.named_parameters()))
    model.train()
    seen = 0
    for i_batch, sampled_batch in enumerate(train_loader):
        volume_batch, label_batch = sampled_batch['image'].cuda(), sampled_batch['label'].cuda()
        assert volume_batch.shape == (4, 1, 96, 96, 96) and label_batch.shape == (4, 1, 96, 96, 96) and label_batch.dtype == torch.int64
        assert bool(torch.isfinite(volume_batch).all())
        outputs = model(volume_batch[:labeled_bs], volume_batch[labeled_bs:])
        assert outputs[0].shape == (2, 16, 96, 96, 96) and bool(torch.isfinite(outputs[0]).all())
        target = label_batch[:labeled_bs].squeeze(1).long()
        assert 0 <= int(target.min()) and int(target.max()) <= 15
        assert torch.nn.functional.cross_entropy(outputs[0], target).isfinite()
        seen += 1
    assert seen == 1
