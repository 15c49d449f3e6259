"""AMOS data feed on the MI355X, through the C ABI (volume_feed_kernel in csrc/kernels/datafeed.h, icl_volume_feed,
icl_amd/dataloaders/amos.py): exactly the numpy restatement of the forward chain (tests/amos_feed_ref.py), at the small sweeps of
test_amos_feed_emu.py and at the trainer's 96^3, and one loader batch through the 16-class model."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import amos_feed_ref as ref  # noqa: E402

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
    return ref.small_store(dev)


@pytest.fixture(scope="module")
def big_store(dev):
    volumes, _ = ref.big_batch()
    return amos_volume_store(volumes, dev)


def test_scalar_path_sweep_on_the_gpu(small_store):
    assert small_store.images[0].is_cuda
    assert ref.check_sweep(small_store, ref.ROI_SCALAR) == 288
    ref.check_padded_voxels(small_store, ref.ROI_SCALAR)


def test_quad_path_sweep_on_the_gpu(small_store):
    assert ref.check_sweep(small_store, ref.ROI_QUAD) == 288
    ref.check_sweep(small_store, ref.ROI_QUAD, misaligned_image=True)       # falls back to one voxel per thread
    ref.check_padded_voxels(small_store, ref.ROI_QUAD)


@pytest.mark.parametrize("roi", [ref.ROI_SCALAR, ref.ROI_QUAD])
def test_inexact_products_are_rounded_twice_on_every_route(dev, roi):
    """mul = 1.1, add = 0.07 on hash-filled volumes, where one rounding and two differ: a multiply-add contracted into an fma in
    volume_feed_gather or the affine path changes these bits.  Plain, device-origin and mixed affine launches."""
    ref.check_twice_rounded_intensity(dev, roi)


def test_batch_of_four_at_the_trainers_roi_equals_the_forward_chain(big_store):
    """(130, 101, 70), (96, 96, 96), (97, 140, 96), (60, 200, 111) -> 96^3: every flip bit, every k, non-zero shifts."""
    _, rows = ref.big_batch()
    want_image, want_label = ref.big_reference()
    got = OnDeviceAugmentAMOS(big_store, ref.BIG_ROI).batch([0, 1, 2, 3], params=rows)
    assert got["image"].shape == (4, 1, 96, 96, 96) and got["label"].shape == (4, 1, 96, 96, 96)
    gi, gl = got["image"].cpu().numpy(), got["label"].cpu().numpy()
    for j in range(4):
        assert np.array_equal(gi[j], want_image[j]), j
        assert np.array_equal(gl[j], want_label[j]), j
    # a captured step's input tensors can be the target: the [B, *roi] label form too
    image = torch.empty((4, 1, 96, 96, 96), device=big_store.device)
    label = torch.empty((4, 96, 96, 96), dtype=torch.int64, device=big_store.device)
    out = OnDeviceAugmentAMOS(big_store, ref.BIG_ROI).batch([0, 1, 2, 3], params=rows, out=(image, label))
    assert out["image"].data_ptr() == image.data_ptr() and out["label"].data_ptr() == label.data_ptr()
    assert torch.equal(image, got["image"]) and torch.equal(label, got["label"][:, 0])


def test_seventeen_samples_are_two_launches_and_runs_repeat_bit_for_bit(small_store):
    indices, rows, want_image, want_label = ref.sweep(ref.ROI_QUAD)
    pick = list(range(5, 5 + 17 * 7, 7))                                     # 17 samples across the sweep
    idx, par = [indices[p] for p in pick], [rows[p] for p in pick]
    feed = OnDeviceAugmentAMOS(small_store, ref.ROI_QUAD)
    first = feed.batch(idx, params=par)
    second = feed.batch(idx, params=par)
    assert first["image"].shape == (17, 1, *ref.ROI_QUAD)
    assert np.array_equal(first["image"].cpu().numpy(), want_image[pick]) and np.array_equal(first["label"].cpu().numpy(), want_label[pick])
    assert torch.equal(first["image"], second["image"]) and torch.equal(first["label"], second["label"])
    assert first["image"].data_ptr() != second["image"].data_ptr()


def test_two_runs_at_the_trainers_roi_are_bit_equal(big_store):
    _, rows = ref.big_batch()
    feed = OnDeviceAugmentAMOS(big_store, ref.BIG_ROI)
    a, b = feed.batch([0, 1, 2, 3], params=rows), feed.batch([0, 1, 2, 3], params=rows)
    assert torch.equal(a["image"], b["image"]) and torch.equal(a["label"], b["label"])


def test_a_loader_batch_feeds_the_16_class_model(big_store):
    """The AMOS trainer's loop head (:216-227) on one AMOSDeviceLoader batch: `model(volume[:2], volume[2:])` of unet_3D_icl with 16
    classes in training mode returns finite logits, and the label passes the trainer's expressions."""
    from icl_amd.networks.net_factory_3d import net_factory_3d
    from icl_amd.utils.hashfill import fill_like_reference_init
    labeled_bs = 2
    np.random.seed(1337)
    feed = OnDeviceAugmentAMOS(big_store, (96, 96, 96))
    train_loader = AMOSDeviceLoader(feed, TwoStreamBatchSampler([0, 1], [2, 3], 4, 2))
    assert len(train_loader) == 1
    model = net_factory_3d(net_type="unet_3D_icl", in_chns=1, class_num=16)
    fill_like_reference_init(list(model.named_parameters()))
    model.train()
    seen = 0
    for i_batch, sampled_batch in enumerate(train_loader):
        volume_batch, label_batch = sampled_batch['image'], sampled_batch['label']
        volume_batch, label_batch = volume_batch.cuda(), label_batch.cuda()
        assert volume_batch.data_ptr() == sampled_batch['image'].data_ptr()        # the .cuda() calls are no-ops
        assert volume_batch.shape == (4, 1, 96, 96, 96) and label_batch.shape == (4, 1, 96, 96, 96) and label_batch.dtype == torch.int64
        outputs = model(volume_batch[:labeled_bs], volume_batch[labeled_bs:])
        assert outputs[0].shape == (2, 16, 96, 96, 96) and bool(torch.isfinite(outputs[0]).all())
        target = label_batch[:labeled_bs].squeeze(1).long()
        assert target.shape == (2, 96, 96, 96) and label_batch[:labeled_bs].long().shape == (2, 1, 96, 96, 96)
        assert 0 <= int(target.min()) and int(target.max()) <= 15
        assert torch.nn.functional.cross_entropy(outputs[0], target).isfinite()
        seen += 1
    assert seen == 1
