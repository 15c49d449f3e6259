"""Affine stage of the BraTS feed on the MI355X, through the C ABI (crop_rotflip_affine_kernel in csrc/kernels/datafeed.h,
icl_crop_rotflip_affine, OnDeviceAugment in icl_amd/dataloaders/brats2019.py): the checks of test_crop_affine_emu.py on the device, and one
case at the trainer's 96^3 against the numpy restatement of DESIGN.md §2 "Affine stage of the BraTS feed" (tests/crop_affine_ref.py)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import crop_affine_ref as ref  # noqa: E402

from icl_amd.dataloaders.amos import affine_matrix  # noqa: E402
from icl_amd.dataloaders.brats2019 import DeviceVolumeStore, OnDeviceAugment  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from icl_amd import _lib
    assert _lib.lib_path().endswith("libicl_hip.so"), "GPU tests must run on the HIP library"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def lib(dev):
    from icl_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize("patch", ref.PATCHES)
@pytest.mark.parametrize("channels", ref.IDENTITY_CHANNELS)
def test_identity_equals_the_plain_entries_on_the_gpu(lib, dev, channels, patch):
    assert ref.check_identity(lib, dev, channels, patch) >= 3 * 12 * 2


@pytest.mark.parametrize("channels", [None, 3])
def test_identity_with_misaligned_outputs_on_the_gpu(lib, dev, channels):
    ref.check_identity(lib, dev, channels, ref.PATCH_QUAD, misaligned=True)


@pytest.mark.parametrize("patch", ref.PATCHES)
@pytest.mark.parametrize("channels", [None, 4])
def test_flag_0_in_a_mixed_launch_is_the_plain_gather_on_the_gpu(lib, dev, channels, patch):
    ref.check_mixed_flags(lib, dev, channels, patch)


@pytest.mark.parametrize("patch", ref.PATCHES)
def test_equals_the_single_channel_affine_kernel_on_the_gpu(lib, dev, patch):
    assert ref.check_against_volume_feed_affine(lib, dev, patch) == 12


@pytest.mark.parametrize("patch", ref.PATCHES)
def test_random_and_dyadic_matrices_equal_the_restatement_on_the_gpu(lib, dev, patch):
    assert ref.check_reference(lib, dev, patch) == 18


@pytest.mark.parametrize("patch", ref.PATCHES)
def test_a_tap_outside_the_volume_is_zero_whatever_the_volume_holds_on_the_gpu(lib, dev, patch):
    ref.check_nonfinite(lib, dev, patch)


def test_the_tiled_thread_mapping_of_the_affine_path_on_the_gpu(lib, dev):
    """Patch (6, 8, 8): identity against the plain entry, a mixed launch, the single-channel kernel (aligned and misaligned outputs on its
    side), the restatement (random, dyadic, misaligned outputs) and non-finite volumes."""
    ref.check_identity(lib, dev, 3, ref.PATCH_TILED)
    ref.check_identity(lib, dev, None, ref.PATCH_TILED, misaligned=True)
    ref.check_mixed_flags(lib, dev, 4, ref.PATCH_TILED)
    assert ref.check_against_volume_feed_affine(lib, dev, ref.PATCH_TILED) == 12
    assert ref.check_against_volume_feed_affine(lib, dev, ref.PATCH_TILED, misaligned_amos=True) == 12
    assert ref.check_reference(lib, dev, ref.PATCH_TILED) == 18
    ref.check_nonfinite(lib, dev, ref.PATCH_TILED)


@pytest.mark.parametrize("patch", ref.PATCHES)
def test_a_single_channel_store_passes_one_channel_on_the_gpu(lib, dev, patch):
    ref.check_single_channel_store(lib, dev, patch)


@pytest.mark.parametrize("patch", ref.PATCHES)
def test_image_against_scipy_on_the_gpu(lib, dev, patch):
    ref.check_scipy(lib, dev, patch)


@pytest.mark.parametrize("channels", [None, 3])
def test_loader_on_the_gpu(dev, monkeypatch, channels):
    ref.check_loader(dev, monkeypatch, channels)


def test_refusals_write_nothing_on_the_gpu(lib, dev):
    ref.check_refusals(lib, dev)


def test_two_samples_of_a_four_channel_volume_at_the_trainers_patch(dev):
    """One (4, 100, 110, 98) volume, patch 96^3, two samples (k = 1 with a flip of axis 0, k = 2 with a flip of axis 1), each with a
    random M (+-0.5 rad, anisotropic zoom 0.7 .. 1.4), through OnDeviceAugment: equal to the restatement on every voxel."""
    shape, patch = (100, 110, 98), (96, 96, 96)
    rng = np.random.RandomState(96)
    image = np.stack([(rng.uniform(-1.0, 3.0, size=shape) + 10.0 * c).astype(np.float32) for c in range(4)])
    label = rng.randint(0, 4, size=shape).astype(np.uint8)
    rows = []
    for k, axis in ((1, 0), (2, 1)):
        row = ref.random_origin_row(rng, shape, k, axis, patch)
        assert row[5:8] == (0, 0, 0)                                     # every extent exceeds the patch: no padding
        rows.append([*row, *affine_matrix(rng.uniform(-0.5, 0.5, 3), rng.uniform(0.7, 1.4, 3)).reshape(-1)])
    got = OnDeviceAugment(DeviceVolumeStore([(image, label)], dev), patch).batch([0, 0], params=rows)
    assert got["image"].shape == (2, 4, 96, 96, 96) and got["label"].shape == (2, 96, 96, 96)
    gi, gl = got["image"].cpu().numpy(), got["label"].cpu().numpy()
    for j, row in enumerate(rows):
        want_image, want_label = ref.crop_affine_chain(image, label, row[:11], row[11:], patch)
        assert np.array_equal(gi[j], want_image), j
        assert np.array_equal(gl[j], want_label), j
        assert (want_image == 0).any() and (want_image != 0).mean() > 0.5   # the rotated patch leaves the volume at its corners only
