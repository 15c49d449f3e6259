"""Intensity stage of the 3-D feed (csrc/kernels/intensity.h, icl_intensity_noise / _blur / _stats / _point, icl_amd/dataloaders/intensity.py)
on the CPU emulation of the kernel sources, against the numpy restatement of DESIGN.md §2 "Intensity stage of the 3-D feed" in
tests/intensity_feed_ref.py; the GPU run is in test_gpu_intensity_feed.py.  Blur, statistics and contrast are compared exactly; noise and
gamma within the bounds derived in intensity_feed_ref.py's docstring; the blur's restatement is compared with scipy itself, bit for bit;
the draws are pinned on the host alone.  Parity with MONAI's and nnU-Net's own code is unpinned (neither is installed)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "hipemu"))
from build_emu import build_emu  # noqa: E402
import intensity_feed_ref as ref  # noqa: E402
import posneg_feed_ref as pref  # noqa: E402

from icl_amd import _lib  # noqa: E402
from icl_amd.dataloaders.amos import OnDeviceAugmentAMOS  # noqa: E402
from icl_amd.dataloaders.brats2019 import OnDeviceAugment  # noqa: E402
from icl_amd.dataloaders.intensity import IntensityAugment, blur_weights, draw_intensity_params  # noqa: E402


@pytest.fixture(scope="module")
def emu(request):
    _lib._use_library_for_tests(build_emu(), host_pointers=True)
    yield "cpu"
    _lib._use_library_for_tests(None)


def test_off_is_off(emu):
    ref.check_off_is_off(emu)


def test_blur_equals_the_restatement(emu):
    assert ref.check_blur(emu) == 2 * (4 + 4 + 3 + 1)


@pytest.mark.parametrize("shape,sigma", ref.SCIPY_CASES)
def test_the_blur_restatement_equals_scipy_bit_for_bit(shape, sigma):
    """The definition IS scipy.ndimage.gaussian_filter(x, sigma, mode="reflect", truncate=4.0) on the fp32 patch; if another scipy
    breaks this equality, that is a finding to report, not a bound to loosen."""
    from scipy import ndimage
    x = ref.patch(shape, 90)
    want = ndimage.gaussian_filter(x, sigma, mode="reflect", truncate=4.0)
    assert want.dtype == np.float32
    got = ref.blur_ref(x, sigma)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (shape, sigma, ref.differing(got, want))
    w, r, _ = ref.blur_weights_ref(sigma)
    assert np.array_equal(blur_weights(sigma), w) and len(w) == r + 1


@pytest.mark.parametrize("shape", ref.SHAPES)
def test_statistics_and_contrast(emu, shape):
    assert ref.check_contrast(emu, shape) == 5


@pytest.mark.parametrize("shape", [ref.SHAPE_SCALAR, ref.SHAPE_QUAD])
def test_noise_against_the_fp64_restatement(emu, shape):
    ref.check_noise(emu, shape)


@pytest.mark.parametrize("shape", [ref.SHAPE_SCALAR, ref.SHAPE_QUAD])
def test_gamma_against_the_fp64_restatement(emu, shape):
    ref.check_gamma(emu, shape)


def test_noise_distribution(emu):
    ref.check_noise_distribution(emu)


def test_whole_chain_through_the_amos_feed_in_two_chunks(emu):
    ref.check_chain_amos(emu)


def test_whole_chain_through_the_brats_and_posneg_feeds(emu):
    ref.check_chain_other_stores(emu)


def test_refusals_return_their_error_without_a_launch(emu):
    ref.check_refusals(emu)


# ---- the draws: host only ---------------------------------------------------------------------------------------------------------------

def test_draws_follow_the_documented_sequence():
    on = dict(noise_prob=1.0, noise_sigma=(0.02, 0.1), noise_clip=2.0, blur_prob=1.0, blur_sigma=(0.5, 1.5), contrast_prob=1.0,
              contrast_range=(0.75, 1.25), gamma_prob=1.0, gamma_range=(0.7, 1.5), invert_prob=0.25)
    # all off: nothing is drawn, the generator is untouched, the rows are the neutral row
    rec = pref.RecordingRNG(1)
    assert draw_intensity_params(rec, 3) == [ref.OFF_ROW] * 3 and rec.calls == []
    rec = pref.RecordingRNG(1)
    assert draw_intensity_params(rec, 2, noise_prob=0, blur_prob=0.0, contrast_prob=0, gamma_prob=0, invert_prob=1.0) == [ref.OFF_ROW] * 2
    assert rec.calls == []
    # all on, two samples: sample after sample, transform after transform; the branch draws of contrast and gamma depend on the values
    rec = pref.RecordingRNG(8)
    rows = draw_intensity_params(rec, 2, **on)
    rng = np.random.RandomState(8)
    want_calls, want_rows = [], []
    for _ in range(2):
        want_calls += [("rand",), ("randint", 0, 2 ** 32), ("uniform", 0.02, 0.1)]
        assert rng.rand() < 1.0
        seed, ns = int(rng.randint(0, 2 ** 32)), rng.uniform(0.02, 0.1)
        want_calls += [("rand",), ("uniform", 0.5, 1.5)]
        assert rng.rand() < 1.0
        bs = rng.uniform(0.5, 1.5)
        want_calls += [("rand",), ("rand",)]
        assert rng.rand() < 1.0
        low = rng.rand() < 0.5
        want_calls += [("uniform", 0.75, 1)] if low else [("uniform", 1, 1.25)]
        f = rng.uniform(0.75, 1) if low else rng.uniform(1, 1.25)
        want_calls += [("rand",), ("rand",), ("rand",)]
        assert rng.rand() < 1.0
        invert = int(rng.rand() < 0.25)
        low = rng.rand() < 0.5
        want_calls += [("uniform", 0.7, 1)] if low else [("uniform", 1, 1.5)]
        g = rng.uniform(0.7, 1) if low else rng.uniform(1, 1.5)
        want_rows.append((1, seed, ns, 2.0, 1, bs, 1, float(np.float32(f)), 1, g, invert))
    assert rec.calls == want_calls and rows == want_rows
    # each transform alone, with fixed sigmas: a single number is not drawn; invert_prob = 0 draws nothing
    rec = pref.RecordingRNG(2)
    (r,) = draw_intensity_params(rec, 1, noise_prob=1.0, noise_sigma=0.1, noise_clip=2)
    assert rec.calls == [("rand",), ("randint", 0, 2 ** 32)] and r[:4] == (1, r[1], 0.1, 2.0) and r[4:] == ref.OFF_ROW[4:]
    rec = pref.RecordingRNG(2)
    (r,) = draw_intensity_params(rec, 1, blur_prob=1.0, blur_sigma=1.25)
    assert rec.calls == [("rand",)] and r == ref.row(blur=1.25)
    rec = pref.RecordingRNG(2)
    (r,) = draw_intensity_params(rec, 1, contrast_prob=1.0, contrast_range=(1.1, 1.3))         # lo >= 1: the first branch is never taken
    assert rec.calls == [("rand",), ("rand",), ("uniform", 1.1, 1.3)] and r[6] == 1 and 1.1 <= r[7] <= 1.3 and r[:6] == ref.OFF_ROW[:6]
    rec = pref.RecordingRNG(2)
    (r,) = draw_intensity_params(rec, 1, gamma_prob=1.0, gamma_range=(0.5, 0.9))
    assert [c[0] for c in rec.calls] == ["rand", "rand", "uniform"] and r[8] == 1 and r[10] == 0 and 0.5 <= r[9] <= 1.0
    # a probability between 0 and 1 decides per sample; a transform that lost its draw draws nothing more
    rows = draw_intensity_params(np.random.RandomState(3), 200, noise_prob=0.3, gamma_prob=0.5, invert_prob=0.5)
    assert 30 < sum(r[0] for r in rows) < 90 and 70 < sum(r[8] for r in rows) < 130 and 0 < sum(r[10] for r in rows) < sum(r[8] for r in rows)
    assert all(r[10] == 0 for r in rows if not r[8])
    rec = pref.RecordingRNG(5)
    draw_intensity_params(rec, 50, blur_prob=0.5, blur_sigma=(0.5, 1.0))
    assert len([c for c in rec.calls if c[0] == "rand"]) == 50 and 10 < len([c for c in rec.calls if c[0] == "uniform"]) < 40


def test_loader_draws_intensity_rows_after_all_geometric_rows():
    """OnDeviceAugmentAMOS.batch with one generator for both: all geometric rows of the batch first, then the intensity rows."""
    class Store:                      # draw() reads the shapes only
        images = [np.zeros(s) for s in ((13, 17, 19), (9, 12, 16))]
        device = None
    rec = pref.RecordingRNG(6)
    stage = IntensityAugment(ref.CHAIN_ROI, rng=rec, noise_prob=1.0, noise_sigma=0.1)
    feed = OnDeviceAugmentAMOS(Store, ref.CHAIN_ROI, rng=rec, rot_prob=0.0, intensity=stage)
    feed.draw([0, 1, 0])
    geometric = len(rec.calls)
    rec2 = pref.RecordingRNG(6)
    OnDeviceAugmentAMOS(Store, ref.CHAIN_ROI, rng=rec2, rot_prob=0.0).draw([0, 1, 0])
    assert rec.calls == rec2.calls                                   # the geometric draws do not change
    stage.draw(3)
    assert rec.calls[geometric:] == [("rand",), ("randint", 0, 2 ** 32)] * 3


def test_constructors_check_every_argument(emu):
    for kw, match in ((dict(noise_prob=1.5), "noise_prob"), (dict(blur_prob=-0.1), "blur_prob"), (dict(contrast_prob=2), "contrast_prob"),
                      (dict(gamma_prob=float("nan")), "gamma_prob"), (dict(invert_prob=1.01), "invert_prob"), (dict(noise_sigma=0.0), "noise_sigma"),
                      (dict(noise_sigma=(0.2, 0.1)), "noise_sigma"), (dict(noise_clip=-1), "noise_clip"), (dict(blur_sigma=(0.5, 3.2)), "blur_sigma"),
                      (dict(blur_sigma=float("inf")), "blur_sigma"), (dict(contrast_range=(0.0, 1.0)), "contrast_range"),
                      (dict(contrast_range=(1.3, 1.2)), "contrast_range"), (dict(gamma_range=(0.7,)), "gamma_range"),
                      (dict(gamma_range=(0.7, float("inf"))), "gamma_range")):
        with pytest.raises(ValueError, match=match):
            IntensityAugment((8, 8, 8), **kw)
    with pytest.raises(TypeError):
        IntensityAugment((8, 8, 8), noise_probability=0.5)
    with pytest.raises(ValueError, match="smallest extent"):
        IntensityAugment((8, 8, 4), blur_prob=0.5, blur_sigma=(0.5, 1.5))
    IntensityAugment((8, 8, 4), blur_prob=0.0, blur_sigma=(0.5, 1.5))             # off: the reach is not an issue
    with pytest.raises(ValueError, match="roi"):
        IntensityAugment((8, 8))
    store = ref.loader_store(emu)
    with pytest.raises(ValueError, match="intensity"):
        OnDeviceAugmentAMOS(store, (8, 8, 12), intensity=IntensityAugment((8, 8, 8)))
    with pytest.raises(ValueError, match="intensity"):
        OnDeviceAugment(store, (8, 8, 8), intensity="noise")
    with pytest.raises(ValueError, match="no intensity stage"):
        OnDeviceAugmentAMOS(store, (8, 8, 12), rot_prob=0.0).batch([0], intensity_params=[ref.OFF_ROW])


def test_apply_refuses_what_it_cannot_take(emu):
    import torch
    stage = IntensityAugment((8, 8, 8))
    good = torch.zeros((2, 1, 8, 8, 8))
    rows = [ref.row(contrast=1.1)] * 2
    for bad in (good.numpy(), good.double(), torch.zeros((2, 1, 8, 8, 9)), torch.zeros((2, 2, 8, 8, 8)), good.transpose(3, 4),
                torch.zeros((2, 1, 8, 8, 16))[..., ::2]):
        with pytest.raises(ValueError, match="contiguous fp32"):
            stage.apply(bad, rows)
    for bad_rows, match in (([rows[0]], "one intensity row"), ([rows[0], rows[0][:10]], "11 expected"), ([rows[0], ref.row(blur=-1.0)], "blur sigma"),
                            ([rows[0], (2,) + ref.OFF_ROW[1:]], "flag"), ([rows[0], (1, 2 ** 32) + ref.OFF_ROW[2:]], "seed"),
                            ([rows[0], ref.row(gamma=(float("nan"), 0))], "gamma")):
        with pytest.raises(ValueError, match=match):
            stage.apply(good, bad_rows)
    assert not good.any()
    _lib._use_library_for_tests(None)                    # the product binding refuses host memory before any pointer travels
    try:
        with pytest.raises(ValueError, match="HIP device"):
            stage.apply(good, rows)
    finally:
        _lib._use_library_for_tests(build_emu(), host_pointers=True)
    with pytest.raises(RuntimeError, match="radius"):    # what the constructor could not see is refused by the launcher
        stage.apply(good, [ref.row(blur=2.2), ref.OFF_ROW])
