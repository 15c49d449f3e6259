"""Affine stage of the BraTS feed (crop_rotflip_affine_kernel in csrc/kernels/datafeed.h, icl_crop_rotflip_affine, OnDeviceAugment in
icl_amd/dataloaders/brats2019.py) on the CPU emulation of the kernel sources, against the plain gather entries, the single-channel affine
kernel on a materialised volume, the numpy restatement of DESIGN.md §2 "Affine stage of the BraTS feed" in tests/crop_affine_ref.py, and
scipy's affine_transform; the GPU run is in test_gpu_crop_affine.py.  Every comparison but scipy's is exact.  Parity with MONAI's
RandAffine is unpinned (MONAI is not installed, and it samples the cropped patch)."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "hipemu"))
from build_emu import build_emu  # noqa: E402
import crop_affine_ref as ref  # noqa: E402

from icl_amd import _lib  # noqa: E402

CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def emu():
    _lib._use_library_for_tests(build_emu(), host_pointers=True)
    yield _lib.lib()
    _lib._use_library_for_tests(None)


@pytest.mark.parametrize("patch", ref.PATCHES)
@pytest.mark.parametrize("channels", ref.IDENTITY_CHANNELS)
def test_identity_equals_the_plain_entries(emu, channels, patch):
    """M = I on every sample: icl_crop_rotflip for a [W,H,D] store (channels None), icl_crop_rotflip_channels for C = 1, 2, 3, 4, 16."""
    assert ref.check_identity(emu, CPU, channels, patch) >= 3 * 12 * 2


@pytest.mark.parametrize("channels", [None, 3])
def test_identity_with_misaligned_outputs_takes_the_scalar_form(emu, channels):
    ref.check_identity(emu, CPU, channels, ref.PATCH_QUAD, misaligned=True)


@pytest.mark.parametrize("patch", ref.PATCHES)
@pytest.mark.parametrize("channels", [None, 4])
def test_flag_0_in_a_mixed_launch_is_the_plain_gather(emu, channels, patch):
    ref.check_mixed_flags(emu, CPU, channels, patch)


@pytest.mark.parametrize("patch", ref.PATCHES)
def test_equals_the_single_channel_affine_kernel_on_the_materialised_volume(emu, patch):
    assert ref.check_against_volume_feed_affine(emu, CPU, patch) == 12


@pytest.mark.parametrize("patch", ref.PATCHES)
def test_random_and_dyadic_matrices_equal_the_restatement(emu, patch):
    assert ref.check_reference(emu, CPU, patch) == 18


@pytest.mark.parametrize("patch", ref.PATCHES)
def test_a_tap_outside_the_volume_is_zero_whatever_the_volume_holds(emu, patch):
    ref.check_nonfinite(emu, CPU, patch)


def test_the_tiled_thread_mapping_of_the_affine_path(emu):
    """Patch (6, 8, 8): identity against the plain entry, a mixed launch, the single-channel kernel (aligned and misaligned outputs on its
    side), the restatement (random, dyadic, misaligned outputs) and non-finite volumes."""
    ref.check_identity(emu, CPU, 3, ref.PATCH_TILED)
    ref.check_identity(emu, CPU, None, ref.PATCH_TILED, misaligned=True)
    ref.check_mixed_flags(emu, CPU, 4, ref.PATCH_TILED)
    assert ref.check_against_volume_feed_affine(emu, CPU, ref.PATCH_TILED) == 12
    assert ref.check_against_volume_feed_affine(emu, CPU, ref.PATCH_TILED, misaligned_amos=True) == 12
    assert ref.check_reference(emu, CPU, ref.PATCH_TILED) == 18
    ref.check_nonfinite(emu, CPU, ref.PATCH_TILED)


@pytest.mark.parametrize("patch", ref.PATCHES)
def test_a_single_channel_store_passes_one_channel(emu, patch):
    ref.check_single_channel_store(emu, CPU, patch)


@pytest.mark.parametrize("patch", ref.PATCHES)
def test_image_against_scipy(emu, patch):
    ref.check_scipy(emu, CPU, patch)


@pytest.mark.parametrize("channels", [None, 3])
def test_loader(emu, monkeypatch, channels):
    """affine_prob = 0 draws, launches and yields what it did; affine_prob = 1 draws behind each sample's crop; 17 samples are two
    launches; bad rows raise before anything travels; the per-channel intensity stage runs behind the affine."""
    ref.check_loader(CPU, monkeypatch, channels)


def test_refusals_write_nothing(emu):
    ref.check_refusals(emu, CPU)


def test_helpers_stay_importable_from_the_amos_module():
    from icl_amd.dataloaders import affine, amos
    for name in ("AFFINE_MAX_ENTRY", "affine_matrix", "_affine_arguments", "_draw_affine", "_affine_suffixes", "_affine_block"):
        assert getattr(amos, name) is getattr(affine, name)
