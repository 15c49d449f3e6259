"""Intensity stage of the 3-D feed on the MI355X, through the C ABI (csrc/kernels/intensity.h, icl_intensity_noise / _blur / _stats /
_point, icl_amd/dataloaders/intensity.py): the checks of test_intensity_feed_emu.py (tests/intensity_feed_ref.py) on the device — blur,
statistics and contrast bit-equal to the numpy restatement of DESIGN.md §2 "Intensity stage of the 3-D feed", noise and gamma within the
bounds derived there —, two samples at the trainer's 96^3, and one loader batch with every transform on."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import intensity_feed_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from icl_amd import _lib
    assert _lib.lib_path().endswith("libicl_hip.so"), "GPU tests must run on the HIP library"
    return torch.device("cuda", 0)


def test_off_is_off_on_the_gpu(dev):
    ref.check_off_is_off(dev)


def test_blur_equals_the_restatement_on_the_gpu(dev):
    assert ref.check_blur(dev) == 24


@pytest.mark.parametrize("shape", ref.SHAPES)
def test_statistics_and_contrast_on_the_gpu(dev, shape):
    assert ref.check_contrast(dev, shape) == 5


@pytest.mark.parametrize("shape", [ref.SHAPE_SCALAR, ref.SHAPE_QUAD])
def test_noise_against_the_fp64_restatement_on_the_gpu(dev, shape):
    ref.check_noise(dev, shape)


@pytest.mark.parametrize("shape", [ref.SHAPE_SCALAR, ref.SHAPE_QUAD])
def test_gamma_against_the_fp64_restatement_on_the_gpu(dev, shape):
    ref.check_gamma(dev, shape)


def test_noise_distribution_on_the_gpu(dev):
    ref.check_noise_distribution(dev)


def test_whole_chain_through_the_amos_feed_in_two_chunks(dev):
    ref.check_chain_amos(dev)


def test_whole_chain_through_the_brats_and_posneg_feeds(dev):
    ref.check_chain_other_stores(dev)


def test_refusals_return_their_error_without_a_launch(dev):
    ref.check_refusals(dev)


def test_two_samples_at_the_trainers_patch(dev):
    """96^3: 64 workgroups of partial sums with 13.5 quads a slot, 864 tiles a strided blur pass, 42 lines a workgroup in the last.  Sample 0
    takes every transform, sample 1 blur and contrast only, which must be exact."""
    shape = ref.SHAPE_BIG
    samples = [ref.patch(shape, 81), ref.patch(shape, 82, 0.0, 1.0)]
    rows = [ref.row(noise=(99, 0.05, 2.0), blur=1.0, contrast=1.2, gamma=(0.8, 1)), ref.row(blur=2.9, contrast=0.8)]
    got, stats = ref.run_stage(dev, samples, rows)
    # sample 1: exact, statistics included
    blurred = ref.blur_ref(samples[1], 2.9)
    mn, mx, mean = ref.stats_ref(blurred)
    assert stats[1, 0] == mn and stats[1, 1] == mx and np.float32(stats[1, 2]).view(np.uint32) == mean.view(np.uint32)
    want, _ = ref.point_ref(blurred, rows[1], (mn, mx, mean))
    assert np.array_equal(got[1].view(np.uint32), want.view(np.uint32))
    # sample 0: the restatement's chain, within gamma's bound
    want, want_stats, slack = ref.chain_ref(samples[0], rows[0])
    diff = np.abs(got[0].astype(np.float64) - want.astype(np.float64))
    print(f"96^3 all transforms: {ref.differing(got[0], want)} of {want.size} voxels differ at all, worst |diff| {diff.max():.3e} "
          f"(one ulp {slack.max():.3e}); stats {stats[0, :3]} vs {want_stats}")
    assert (diff <= slack).all()
    assert abs(float(stats[0, 2]) - float(want_stats[2])) <= 2.0 ** -23 * float(np.abs(want).max())
