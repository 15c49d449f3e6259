"""Simulated low resolution of the 3-D feed's intensity stage on the MI355X, through the C ABI (intensity_lowres_kernel<1> / <4> and
intensity_lowres_copy_kernel<1> / <4> of csrc/kernels/intensity.h, icl_intensity_lowres, icl_amd/dataloaders/intensity.py): the checks of
test_lowres_feed_emu.py (tests/lowres_feed_ref.py) on the device, BIT-EQUAL to the numpy restatement of DESIGN.md §2 "Intensity stage of
the 3-D feed", and two samples at the trainer's 96^3."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import intensity_feed_ref as ref  # noqa: E402
import lowres_feed_ref as lref  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from icl_amd import _lib
    assert _lib.lib_path().endswith("libicl_hip.so"), "GPU tests must run on the HIP library"
    return torch.device("cuda", 0)


def test_two_samples_per_shape_equal_the_restatement_bit_for_bit_on_the_gpu(dev):
    assert lref.check_samples(dev) == 20


def test_mixed_batch_leaves_the_other_samples_alone_on_the_gpu(dev):
    lref.check_mixed_batch(dev)


def test_whole_chain_through_the_amos_feed_in_two_chunks_on_the_gpu(dev):
    lref.check_chain_amos(dev)


def test_whole_chain_through_the_brats_and_posneg_feeds_on_the_gpu(dev):
    lref.check_chain_other_stores(dev)


def test_off_is_off_on_the_gpu(dev):
    lref.check_off_is_off(dev)


def test_refusals_return_their_error_without_a_launch_on_the_gpu(dev):
    lref.check_refusals(dev)


def test_two_samples_at_the_trainers_patch(dev):
    """96^3, two samples: one anisotropic, low extents (48, 61, 96) (axis 2 left alone), and one off.  864 workgroups a sample, 221,184
    quads; bit-equal to the restatement, and the sample that is off is untouched although the scratch buffer held NaN."""
    shape = lref.SHAPE_BIG
    samples = [ref.patch(shape, 81), ref.patch(shape, 82, 0.0, 1.0)]
    low = (48, 61, 96)
    rows = [lref.row(lowres=lref.zooms_for(shape, low)), lref.row()]
    got, _, _ = lref.run_stage(dev, samples, rows)
    want = lref.lowres_ref(samples[0], low)
    assert lref.same_bits(got[0], want), ref.differing(got[0], want)
    assert lref.same_bits(got[1], samples[1])
    assert ref.differing(got[0], samples[0]) > want.size // 2
