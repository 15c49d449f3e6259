"""Multi-modal volumes, what needs no kernel: the host transforms on a channel-first image, the BraTS validation loop in its ATen form
on a channel-first case, and the networks' constructors at in_channels = 4.  References: tests/multimodal_feed_ref.py."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import multimodal_feed_ref as ref  # noqa: E402

from icl_amd.dataloaders.brats2019 import CenterCrop, RandomCrop, RandomRotFlip, ToTensor  # noqa: E402


def _case(shape, channels, seed):
    rng = np.random.RandomState(seed)
    image = rng.randn(*((channels,) if channels else ()), *shape).astype(np.float32)
    label = rng.randint(0, 4, size=shape).astype(np.uint8)
    return image, label


def _chain(sample, patch):
    return ToTensor()(RandomCrop(patch)(RandomRotFlip()(sample)))


@pytest.mark.parametrize("patch", [(6, 6, 5), (6, 6, 8), (10, 10, 10)])      # no padding, depth <= patch, every axis <= patch
def test_transforms_on_a_channel_first_image_equal_the_3d_classes_per_channel(patch):
    image, label = _case((9, 7, 8), 3, 1)
    for seed in range(12):
        np.random.seed(seed)
        got = _chain({"image": image, "label": label}, patch)
        after = np.random.randint(0, 1 << 30)                      # the state of the generator behind the chain
        assert got["image"].shape == (3, *patch) and got["image"].dtype == torch.float32
        assert got["label"].shape == patch and got["label"].dtype == torch.int64
        for c in range(3):
            np.random.seed(seed)
            one = _chain({"image": image[c], "label": label}, patch)
            assert np.random.randint(0, 1 << 30) == after          # the same number of draws
            assert one["image"].shape == (1, *patch)
            assert torch.equal(one["image"][0], got["image"][c]) and torch.equal(one["label"], got["label"])


def test_3d_results_are_the_numpy_chain_of_the_reference():
    """A [W,H,D] sample through the classes is what the reference's lines do: rot90 / flip on axes (0, 1), pad, window."""
    image, label = _case((9, 7, 8), None, 2)
    patch = (6, 6, 8)
    for seed in range(8):
        np.random.seed(seed)
        got = _chain({"image": image, "label": label}, patch)
        np.random.seed(seed)
        k, axis = np.random.randint(0, 4), np.random.randint(0, 2)
        im, lb = (np.flip(np.rot90(v, k), axis=axis).copy() for v in (image, label))
        if min(im.shape[a] - patch[a] for a in range(3)) <= 0:
            pw = [(max((patch[a] - im.shape[a]) // 2 + 3, 0),) * 2 for a in range(3)]
            im, lb = np.pad(im, pw, mode="constant"), np.pad(lb, pw, mode="constant")
        o = [np.random.randint(0, im.shape[a] - patch[a]) for a in range(3)]
        sl = tuple(slice(o[a], o[a] + patch[a]) for a in range(3))
        assert np.array_equal(got["image"][0].numpy(), im[sl]) and np.array_equal(got["label"].numpy(), lb[sl].astype(np.int64))


def test_center_crop_keeps_the_channel_axis():
    image, label = _case((9, 7, 8), 2, 3)
    for patch in ((6, 6, 5), (10, 10, 10)):
        got = CenterCrop(patch)({"image": image, "label": label})
        assert got["image"].shape == (2, *patch) and got["label"].shape == patch
        for c in range(2):
            one = CenterCrop(patch)({"image": image[c], "label": label})
            assert np.array_equal(one["image"], got["image"][c]) and np.array_equal(one["label"], got["label"])


# ---- validation --------------------------------------------------------------------------------------------------------------------

def test_single_case_on_the_cpu_takes_a_channel_first_image():
    """_single_case_on_device in its ATen form: a [2, 20, 18, 17] case, patch 16^3 and stride 8 (the last window of every axis is
    clamped), with a stand-in net that is a fixed per-voxel function of both channels, against the numpy restatement of the window
    loop; the windows the net saw carry both channels."""
    from icl_amd.val_3D import _single_case_on_device, test_single_case_base
    patch = (16, 16, 16)
    image = ref.validation_case((2, 20, 18, 17))
    net = ref.PerVoxelNet()
    label, score = _single_case_on_device(net, "unet_3D", image, 8, 8, patch, num_classes=3)
    want, windows = ref.window_loop_reference(image, patch, 8, 8)
    assert label.shape == (20, 18, 17) and label.dtype == torch.int64 and score.shape == (3, 20, 18, 17)
    assert np.array_equal(label.numpy(), want)
    assert len(np.unique(want)) == 3
    assert sum(s[0] for s in net.seen) == windows and all(s[1:] == (2, *patch) for s in net.seen)
    assert np.array_equal(test_single_case_base(net, "unet_3D", image, 8, 8, patch, num_classes=3), want)
    with pytest.raises(ValueError, match="a case is an image"):
        _single_case_on_device(net, "unet_3D", image[None], 8, 8, patch, num_classes=3)


def test_single_case_on_a_3d_image_is_what_it_was():
    from icl_amd.val_3D import _single_case_on_device
    patch = (16, 16, 16)
    for shape in ((20, 18, 17), (12, 18, 17)):                       # the second: W below the patch, padded 2 + 2
        image = ref.validation_case(shape, seed=4)
        net = ref.PerVoxelNet()
        label, _ = _single_case_on_device(net, "unet_3D", image, 8, 8, patch, num_classes=3)
        want, _ = ref.window_loop_reference(image, patch, 8, 8)
        assert np.array_equal(label.numpy(), want) and all(s[1:] == (1, *patch) for s in net.seen)
        # a [1,W,H,D] case is the same case
        again, _ = _single_case_on_device(ref.PerVoxelNet(), "unet_3D", image[None], 8, 8, patch, num_classes=3)
        assert torch.equal(again, label)


def test_all_case_base_scores_a_channel_first_case():
    from icl_amd.val_3D import test_all_case_base
    image = ref.validation_case((2, 20, 18, 17))
    want, _ = ref.window_loop_reference(image, (16, 16, 16), 8, 8)
    metrics = test_all_case_base(ref.PerVoxelNet(), "unet_3D", None, num_classes=3, patch_size=(16, 16, 16), stride_xy=8, stride_z=8,
                                 cases=[(image, want.astype(np.uint8))])
    assert len(metrics) == 2 and all(abs(m[0][0] - 1.0) < 1e-12 for m in metrics)      # the prediction scored against itself: Dice 1


# ---- networks ----------------------------------------------------------------------------------------------------------------------

def test_models_are_built_with_four_input_channels():
    """Construction only (the factory needs a HIP device: tests/test_gpu_multimodal.py): the first convolution of the U-Net and the
    two modules of SwinUNETR that see the input, PatchEmbed and encoder1, take the four channels."""
    from icl_amd.networks.swinunetr_icl import SwinUNETR_icl
    from icl_amd.networks.unet_3D_icl import unet_3D_icl
    net = unet_3D_icl(n_classes=2, in_channels=4, icl_in_resolutions=(2, 4, 8))
    assert dict(net.named_parameters())["conv1.conv1.0.weight"].shape == (16, 4, 3, 3, 3)
    swin = SwinUNETR_icl(img_size=(32, 32, 32), in_channels=4, out_channels=2, feature_size=12)
    seen = [k for k, v in swin.named_parameters() if v.dim() == 5 and v.shape[:2] == (12, 4)]
    assert seen == ["swinViT.patch_embed.proj.weight", "encoder1.layer.conv1.conv.weight", "encoder1.layer.conv3.conv.weight"], seen
