"""Affine stage of the 3-D feed (volume_feed_affine_kernel in csrc/kernels/datafeed.h, icl_volume_feed_affine /
icl_volume_feed_affine_origins, icl_amd/dataloaders/amos.py) on the CPU emulation of the kernel sources, against the numpy restatement of
DESIGN.md §2 "Affine stage of the 3-D feed" in tests/affine_feed_ref.py; the GPU run is in test_gpu_affine_feed.py.  Every comparison
with the restatement is exact; scipy's affine_transform is an independent cross-check with the bounds stated at its test; the draws are
pinned on the host alone.  Parity with MONAI's RandAffine is unpinned (MONAI is not installed, and it samples the cropped patch)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "hipemu"))
from build_emu import build_emu  # noqa: E402
import amos_feed_ref as aref  # noqa: E402
import affine_feed_ref as ref  # noqa: E402
import posneg_feed_ref as pref  # noqa: E402

from icl_amd import _lib  # noqa: E402
from icl_amd.dataloaders.amos import (OnDeviceAugmentAMOS, affine_matrix, draw_amos_params, draw_posneg_params)  # noqa: E402


@pytest.fixture(scope="module")
def emu_library():
    _lib._use_library_for_tests(build_emu(), host_pointers=True)
    yield
    _lib._use_library_for_tests(None)


@pytest.fixture(scope="module")
def small_store(emu_library):
    return aref.small_store("cpu")


@pytest.fixture(scope="module")
def cube_store(emu_library):
    return ref.cube_store("cpu")


@pytest.fixture(scope="module")
def random_store(emu_library):
    return ref.random_store("cpu")


@pytest.mark.parametrize("roi", [ref.ROI_SCALAR, ref.ROI_QUAD])
def test_identity_equals_the_plain_feed(small_store, roi):
    assert ref.check_identity(small_store, roi) == 3 * 8 * 4 * 3


def test_proper_signed_permutations_equal_transpose_and_flip(cube_store):
    ref.check_signed_permutations(cube_store)


def test_dyadic_zooms_pin_half_to_even_and_the_half_weights(cube_store):
    ref.check_dyadic_zooms(cube_store)


@pytest.mark.parametrize("roi", ref.RANDOM_ROIS)
def test_random_matrices_equal_the_restatement_on_both_kernels(random_store, roi):
    assert ref.check_random(random_store, roi) == 24


@pytest.mark.parametrize("roi", ref.RANDOM_ROIS)
def test_random_matrices_against_scipy(random_store, roi):
    """Independent cross-check: scipy.ndimage.affine_transform(matrix=M, offset=t - M ctr, output_shape=roi) of the random cases (no
    flips, no quarter turn, no intensity term).  Image, order 1, grid-constant, cval 0, on the float64 image: scipy keeps the sum in
    double, the kernel rounds it once to fp32, so the difference is at most 2^-23 max|image|.  Label, order 0: equal on every voxel
    whose coordinates are farther than 1e-9 from a rounding tie; at most 0.1 % of the voxels may be left out that way."""
    from scipy import ndimage
    cases = ref.random_cases(roi, True)
    got_image, got_label = ref.run_cases(random_store, roi, list(cases))
    left_out = total = 0
    for j, (v, row, M) in enumerate(cases):
        image, label = ref.random_volume(v)
        M = np.asarray(M).reshape(3, 3)
        ctr = (np.asarray(roi, dtype=np.float64) - 1) / 2
        t = np.asarray(row[3:6], dtype=np.float64) - np.asarray(row[9:12], dtype=np.float64) + ctr
        offset = t - M @ ctr
        want = ndimage.affine_transform(image.astype(np.float64), M, offset=offset, output_shape=roi, order=1, mode="grid-constant", cval=0.0)
        worst = float(np.abs(got_image[j, 0].astype(np.float64) - want).max())
        bound = 2.0 ** -23 * float(np.abs(image).max())
        print(f"case {j}: image |diff| {worst:.3e} (bound {bound:.3e})")
        assert worst <= bound, (j, worst, bound)
        want_label = ndimage.affine_transform(label, M, offset=offset, output_shape=roi, order=0, mode="grid-constant", cval=0)
        p = np.stack(np.meshgrid(*[np.arange(r, dtype=np.float64) for r in roi], indexing="ij"))
        x = np.tensordot(M, p, axes=1) + offset[:, None, None, None]
        clear = (np.abs(x - np.floor(x) - 0.5) > 1e-9).all(axis=0)
        assert np.array_equal(got_label[j, 0][clear], want_label[clear].astype(np.int64)), j
        left_out += int((~clear).sum())
        total += clear.size
    print(f"label voxels left out near a tie: {left_out} of {total}")
    assert left_out <= total / 1000


@pytest.mark.parametrize("roi", ref.ROIS)
def test_nonfinite_voxels_count_only_where_a_tap_is_inside(emu_library, roi):
    assert ref.check_nonfinite(ref.nonfinite_store("cpu"), roi) == 24


def test_mixed_batch_of_17_is_two_launches(random_store):
    ref.check_mixed_batch(random_store)


def test_device_origins_equal_host_origins_and_are_clamped(emu_library):
    ref.check_device_origins("cpu")


def test_refusals_write_nothing(small_store):
    ref.check_refusals(small_store)


# ---- the draws: host only ---------------------------------------------------------------------------------------------------------------

def test_draws_without_an_affine_are_todays_draws():
    """Defaults and an explicit affine_prob = 0: the rows of the documented pre-affine sequence, the generator left in the same state."""
    shape, roi = (13, 17, 19), (6, 6, 8)
    for seed in range(5):
        for kw in ({}, dict(affine_prob=0), dict(affine_prob=0.0, rotate_range=0.3, zoom_range=(0.8, 1.2), zoom_isotropic=False)):
            tail = dict(flip_prob=0.5, rot_prob=0.5, scale_factor=0.1, scale_prob=0.5)
            a, b = np.random.RandomState(seed), np.random.RandomState(seed)
            row = draw_amos_params(shape, roi, a, **tail, **kw)
            # the documented sequence of draw_amos_params before the stage existed, restated
            origin = [int(b.randint(0, n - r + 1)) for n, r in zip(shape, roi)]
            flip = sum(int(b.rand() < 0.5) << ax for ax in range(3))
            k = int(b.randint(3)) + 1 if b.rand() < 0.5 else 0
            mul = np.float32(1 + b.uniform(-0.1, 0.1)) if b.rand() < 0.5 else np.float32(1)
            add = np.float32(b.uniform(-0.1, 0.1)) if b.rand() < 0.5 else np.float32(0)
            assert row == (*shape, *origin, *roi, 0, 0, 0, flip, k, float(mul), float(add)) and len(row) == 16
            assert a.rand() == b.rand()                                   # same state afterwards
            rec = pref.RecordingRNG(seed)
            rows = draw_posneg_params(shape, roi, 1400, 900, rec, **tail, **kw)
            want_rows, want_calls = pref.documented_draws(seed, shape, roi, 1400, 900, **tail)
            assert rows == want_rows and rec.calls == want_calls and all(len(r) == 18 for r in rows)


def test_draws_with_an_affine_follow_the_documented_sequence():
    shape, roi = (13, 17, 19), (6, 6, 8)
    for isotropic, zooms in ((True, 1), (False, 3)):
        rec = pref.RecordingRNG(4)
        quiet = dict(flip_prob=0.0, rot_prob=0.0, shift_prob=0.0)
        row = draw_amos_params(shape, roi, rec, affine_prob=1.0, rotate_range=(0.1, 0.2, 0.3), zoom_range=(0.7, 1.4), zoom_isotropic=isotropic, **quiet)
        assert len(row) == 25
        assert rec.calls[:3] == [("randint", 0, 8), ("randint", 0, 12), ("randint", 0, 12)]                         # the crop
        affine = rec.calls[3:3 + 1 + 3 + zooms]
        assert affine == [("rand",), ("uniform", -0.1, 0.1), ("uniform", -0.2, 0.2), ("uniform", -0.3, 0.3)] + [("uniform", 0.7, 1.4)] * zooms
        assert rec.calls[3 + 1 + 3 + zooms:] == [("rand",)] * 5                                                     # three flips, rotation, shift
        # the same values from a generator of its own
        rng = np.random.RandomState(4)
        for n, r in zip(shape, roi):
            rng.randint(0, n - r + 1)
        assert rng.rand() < 1.0
        theta = [rng.uniform(-r, r) for r in (0.1, 0.2, 0.3)]
        z = np.array([rng.uniform(0.7, 1.4) for _ in range(zooms)] * (3 if isotropic else 1))
        M = np.array(row[16:]).reshape(3, 3)
        assert np.array_equal(M, affine_matrix(theta, z))
        rot = M @ np.diag(z)
        assert np.abs(rot @ rot.T - np.eye(3)).max() <= 1e-14 and abs(np.linalg.det(rot) - 1) <= 1e-14
        # one number for rotate_range means all three axes; the probability decides between 16 and 25 values
        rec = pref.RecordingRNG(4)
        draw_amos_params(shape, roi, rec, affine_prob=1.0, rotate_range=0.25, zoom_isotropic=isotropic, **quiet)
        assert rec.calls[4:7] == [("uniform", -0.25, 0.25)] * 3
    lengths = {len(draw_amos_params(shape, roi, np.random.RandomState(s), affine_prob=0.5, rotate_range=0.3)) for s in range(20)}
    assert lengths == {16, 25}
    # pos/neg: all centres first, then per crop the affine draw in front of its tail; rows of 18 or 27
    rec = pref.RecordingRNG(6)
    rows = draw_posneg_params(shape, roi, 1400, 900, rec, num_samples=3, affine_prob=1.0, rotate_range=0.3, zoom_range=(0.9, 1.1),
                              flip_prob=0.0, rot_prob=0.0, shift_prob=0.0)
    assert [len(r) for r in rows] == [27] * 3
    assert [c[0] for c in rec.calls[:6]] == ["rand", "randint"] * 3
    per_crop = [("rand",)] + [("uniform", -0.3, 0.3)] * 3 + [("uniform", 0.9, 1.1)] + [("rand",)] * 5
    assert rec.calls[6:] == per_crop * 3
    lengths = {len(r) for s in range(10) for r in draw_posneg_params(shape, roi, 14, 9, np.random.RandomState(s), affine_prob=0.5)}
    assert lengths == {18, 27}


def test_rotations_are_right_handed_about_their_axes():
    for a in range(3):
        theta = [0.0, 0.0, 0.0]
        theta[a] = np.pi / 2
        M = affine_matrix(theta, 1.0)
        b, c = (a + 1) % 3, (a + 2) % 3
        e = np.eye(3)
        assert np.allclose(M @ e[a], e[a], atol=1e-15) and np.allclose(M @ e[b], e[c], atol=1e-15) and np.allclose(M @ e[c], -e[b], atol=1e-15)
    assert np.array_equal(affine_matrix((0, 0, 0), (2.0, 4.0, 0.5)), np.diag([0.5, 0.25, 2.0]))
    assert np.array_equal(affine_matrix((0, 0, 0), 2.0), np.diag([0.5, 0.5, 0.5]))
    t = (0.3, -0.2, 0.4)
    assert np.allclose(affine_matrix(t, 1.0), affine_matrix((t[0], 0, 0), 1) @ affine_matrix((0, t[1], 0), 1) @ affine_matrix((0, 0, t[2]), 1), atol=1e-15)


def test_constructor_checks_the_affine_keywords(small_store):
    for kw, match in ((dict(affine_prob=1.5), "affine_prob"), (dict(affine_prob=-0.1), "affine_prob"),
                      (dict(rotate_range=(0.1, -0.1, 0.1)), "rotate_range"), (dict(rotate_range=(0.1, 0.2)), "rotate_range"),
                      (dict(zoom_range=(0.0, 1.0)), "zoom_range"), (dict(zoom_range=(1.2, 1.1)), "zoom_range"),
                      (dict(zoom_range=(1.0, float("inf"))), "zoom_range")):
        with pytest.raises(ValueError, match=match):
            OnDeviceAugmentAMOS(small_store, ref.ROI_QUAD, **kw)
    index = pref.ForegroundIndex(small_store)
    with pytest.raises(ValueError, match="zoom_range"):
        pref.OnDeviceAugmentPosNeg(small_store, index, ref.ROI_QUAD, zoom_range=(2.0, 1.0))
    with pytest.raises(TypeError):
        OnDeviceAugmentAMOS(small_store, ref.ROI_QUAD, affine_probability=0.5)
    feed = OnDeviceAugmentAMOS(small_store, ref.ROI_QUAD, rng=np.random.RandomState(2), affine_prob=1.0, rotate_range=0.4, zoom_range=(0.8, 1.25))
    got = feed.batch([0, 1, 2])
    assert got["image"].shape == (3, 1, *ref.ROI_QUAD) and bool(np.isfinite(got["image"].numpy()).all())
