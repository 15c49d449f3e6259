"""Simulated low resolution of the 3-D feed's intensity stage (intensity_lowres_kernel in csrc/kernels/intensity.h, icl_intensity_lowres,
icl_amd/dataloaders/intensity.py) on the CPU emulation of the kernel sources, against the numpy restatement in tests/lowres_feed_ref.py,
BIT FOR BIT; the GPU run is in test_gpu_lowres_feed.py.  Host only: the restatement's indices and weights against torch's own 1-D
``interpolate`` for every 1 <= L <= R <= 128 (exactly), the restatement against torch's whole chain (derived bound), and the draws.
Parity with nnU-Net's SimulateLowResolutionTransform class is unpinned (batchgeneratorsv2 is not installed); what is pinned is the
``interpolate`` chain that class is made of."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "hipemu"))
from build_emu import build_emu  # noqa: E402
import intensity_feed_ref as ref  # noqa: E402
import lowres_feed_ref as lref  # noqa: E402
import posneg_feed_ref as pref  # noqa: E402

from icl_amd import _lib  # noqa: E402
from icl_amd.dataloaders.intensity import IntensityAugment, draw_intensity_params, lowres_extents  # noqa: E402


@pytest.fixture(scope="module")
def emu(request):
    _lib._use_library_for_tests(build_emu(), host_pointers=True)
    yield "cpu"
    _lib._use_library_for_tests(None)


# ---- host only: the formulas and the restatement against torch -----------------------------------------------------------------------------

def test_indices_and_weights_equal_torchs_for_every_pair_of_extents():
    """For every 1 <= L <= R <= 128: ``near`` against interpolate(mode="nearest-exact") of a ramp, and the fp32 weights read back through
    the two 0 / 1 parity probes x = (arange(L) % 2 == k) of interpolate(mode="linear"): with such inputs both products of w0 x[i0] + w1 x[i1]
    are exact, so torch's output shows its indices' parities and its weights themselves."""
    import torch.nn.functional as F
    bad_near = bad_weight = pairs = 0
    for R in range(1, 129):
        ramp = torch.arange(R, dtype=torch.float32).view(1, 1, R)
        for L in range(1, R + 1):
            pairs += 1
            near = lref.near_ref(L, R)
            got = F.interpolate(ramp, size=L, mode="nearest-exact")[0, 0].numpy()
            bad_near += int((got != near.astype(np.float32)).sum())
            i0, i1, w0, w1 = lref.taps_ref(L, R)
            assert i0.min() >= 0 and i1.max() <= L - 1 and near.min() >= 0 and near.max() <= R - 1
            for k in (0, 1):
                probe = (torch.arange(L) % 2 == k).to(torch.float32).view(1, 1, L)
                got = F.interpolate(probe, size=R, mode="linear", align_corners=False)[0, 0].numpy()
                want = ((w0 * (i0 % 2 == k).astype(np.float32)).astype(np.float32) + (w1 * (i1 % 2 == k).astype(np.float32)).astype(np.float32))
                bad_weight += int((got.view(np.uint32) != want.astype(np.float32).view(np.uint32)).sum())
    print(f"{pairs} pairs (L, R): {bad_near} indices and {bad_weight} weights differ from torch {torch.__version__}")
    assert pairs == 128 * 129 // 2 and bad_near == 0 and bad_weight == 0


TORCH_CASES = [((7, 9, 10), (4, 4, 5)), ((8, 12, 16), (4, 6, 8)), ((9, 11, 13), (5, 9, 7)), ((16, 16, 16), (1, 16, 5)), ((32, 32, 32), (31, 17, 2)),
               ((40, 40, 44), (13, 40, 29)), ((5, 64, 3), (5, 21, 1)), ((64, 48, 32), (20, 47, 11)), ((96, 96, 96), (48, 61, 96)),
               ((96, 96, 96), (29, 48, 77))]


def test_the_restatement_equals_torchs_whole_chain_within_the_derived_bound():
    """interpolate(size=L, mode="nearest-exact") then interpolate(size=R, mode="trilinear") on the CPU.  The bound is derived: torch's
    fp32 chain is three 1-D interpolations of at most three roundings each (two products, one sum), each at most 2^-24 of the largest
    magnitude, nine in all; the restatement rounds once: 10 * 2^-24 * max|x|.  If another torch breaks it, that is a finding to report,
    not a bound to loosen."""
    worst = 0.0
    for j, (shape, low) in enumerate(TORCH_CASES):
        x = ref.patch(shape, 120 + j, -0.75 if j % 2 else 10.0, 1.25 if j % 2 else 11.0)
        want = lref.torch_chain(x, low)
        got = lref.lowres_ref(x, low)
        unit = 2.0 ** -24 * float(np.abs(x).max())
        units = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max()) / unit
        print(f"{shape} -> {low}: worst |restatement - torch| = {units:.2f} x 2^-24 max|x|")
        worst = max(worst, units)
        assert units <= 10.0, (shape, low, units)
        assert got.min() >= x.min() and got.max() <= x.max()
    print(f"worst over {len(TORCH_CASES)} cases: {worst:.2f} of the 10 units allowed")


def test_draws_follow_the_documented_sequence():
    # one shared zoom: rand, then ONE uniform, between blur's draws and contrast's
    rec = pref.RecordingRNG(8)
    rows = draw_intensity_params(rec, 2, blur_prob=1.0, blur_sigma=(0.5, 1.5), lowres_prob=1.0, lowres_zoom=(0.4, 0.8), contrast_prob=1.0,
                                 contrast_range=(1.1, 1.3))
    rng = np.random.RandomState(8)
    want_calls, want_rows = [], []
    for _ in range(2):
        want_calls += [("rand",), ("uniform", 0.5, 1.5), ("rand",), ("uniform", 0.4, 0.8), ("rand",), ("rand",), ("uniform", 1.1, 1.3)]
        assert rng.rand() < 1.0
        bs = rng.uniform(0.5, 1.5)
        assert rng.rand() < 1.0
        z = rng.uniform(0.4, 0.8)
        rng.rand(), rng.rand()
        f = rng.uniform(1.1, 1.3)
        want_rows.append((0, 0, 1.0, 0.0, 1, bs, 1, float(np.float32(f)), 0, 1.0, 0, 1, z, z, z))
    assert rec.calls == want_calls and rows == want_rows
    # three per-axis zooms, in increasing axis order, whatever the order of lowres_axes
    rec = pref.RecordingRNG(9)
    (r,) = draw_intensity_params(rec, 1, lowres_prob=1.0, lowres_zoom=(0.25, 0.75), lowres_per_axis=True, lowres_axes=(2, 0, 1))
    rng = np.random.RandomState(9)
    rng.rand()
    z = [rng.uniform(0.25, 0.75) for _ in range(3)]
    assert rec.calls == [("rand",)] + [("uniform", 0.25, 0.75)] * 3 and r == ref.OFF_ROW + (1, z[0], z[1], z[2]) and len(set(z)) == 3
    # lowres_axes = (0, 1): axis 2 keeps the zoom 1 and draws nothing
    rec = pref.RecordingRNG(10)
    (r,) = draw_intensity_params(rec, 1, lowres_prob=1.0, lowres_per_axis=True, lowres_axes=(0, 1))
    assert rec.calls == [("rand",), ("uniform", 0.5, 1.0), ("uniform", 0.5, 1.0)] and r[11] == 1 and r[14] == 1.0 and r[12] != r[13]
    rec = pref.RecordingRNG(10)
    (r,) = draw_intensity_params(rec, 1, lowres_prob=1.0, lowres_axes=(0, 1))
    assert rec.calls == [("rand",), ("uniform", 0.5, 1.0)] and r[12] == r[13] < 1.0 and r[14] == 1.0
    # a lost draw draws no zoom, and the row still has 15 values
    rec = pref.RecordingRNG(11)
    rows = draw_intensity_params(rec, 40, lowres_prob=0.25)
    on = sum(r[11] for r in rows)
    assert 2 < on < 20 and len([c for c in rec.calls if c[0] == "rand"]) == 40 and len([c for c in rec.calls if c[0] == "uniform"]) == on
    assert all(len(r) == 15 and (r[11] == 1 or r[11:] == lref.LOWRES_OFF) for r in rows)
    # lowres_prob = 0: nothing is drawn, rows of 11, whatever the other low-resolution keywords say
    rec = pref.RecordingRNG(1)
    assert draw_intensity_params(rec, 3, lowres_prob=0, lowres_zoom=(0.1, 0.2), lowres_per_axis=True, lowres_axes=(1,)) == [ref.OFF_ROW] * 3
    assert rec.calls == []
    stage = IntensityAugment((8, 8, 12), rng=pref.RecordingRNG(1), noise_prob=1.0, lowres_prob=0.0)
    assert stage.enabled and all(len(r) == 11 for r in stage.draw(2))
    assert IntensityAugment((8, 8, 12), lowres_prob=0.5).enabled


def test_lowres_extents_rounds_ties_to_even_and_never_below_one():
    assert lowres_extents((5, 7, 9), (0.5, 0.5, 0.5)) == (2, 4, 4)                 # 2.5 -> 2, 3.5 -> 4, 4.5 -> 4
    assert lowres_extents((96, 96, 96), (0.5, 0.637, 1.0)) == (48, 61, 96)
    assert lowres_extents((3, 1, 96), (0.1, 0.4, 0.004)) == (1, 1, 1)              # 0.3, 0.4, 0.384: never 0
    assert lowres_extents((12, 12, 12), (0.125, 0.2083, 0.2084)) == (2, 2, 3)      # 1.5 -> 2, 2.4996 -> 2, 2.5008 -> 3
    assert all(isinstance(v, int) for v in lowres_extents((8, 8, 12), (0.5, 0.75, 1.0)))
    from compat.dataloaders.intensity import lowres_extents as exported
    assert exported is lowres_extents


def test_constructor_checks_the_new_keywords():
    for kw, match in ((dict(lowres_prob=1.5), "lowres_prob"), (dict(lowres_prob=float("nan")), "lowres_prob"), (dict(lowres_zoom=(0.0, 1.0)), "lowres_zoom"),
                      (dict(lowres_zoom=(0.5, 1.01)), "lowres_zoom"), (dict(lowres_zoom=(0.8, 0.5)), "lowres_zoom"), (dict(lowres_zoom=0.5), "lowres_zoom"),
                      (dict(lowres_zoom=(0.5, float("nan"))), "lowres_zoom"), (dict(lowres_axes=()), "lowres_axes"), (dict(lowres_axes=(0, 0)), "lowres_axes"),
                      (dict(lowres_axes=(0, 3)), "lowres_axes"), (dict(lowres_axes=(0.5,)), "lowres_axes"), (dict(lowres_axes=1), "lowres_axes")):
        with pytest.raises(ValueError, match=match):
            IntensityAugment((8, 8, 8), **kw)


# ---- on the emulator: the checks the GPU runs too ---------------------------------------------------------------------------------------

def test_two_samples_per_shape_equal_the_restatement_bit_for_bit(emu):
    assert lref.check_samples(emu) == 2 * (3 * 3 + 1)


def test_mixed_batch_leaves_the_other_samples_alone(emu):
    lref.check_mixed_batch(emu)


def test_whole_chain_through_the_amos_feed_in_two_chunks(emu):
    lref.check_chain_amos(emu)


def test_whole_chain_through_the_brats_and_posneg_feeds(emu):
    lref.check_chain_other_stores(emu)


def test_off_is_off(emu):
    lref.check_off_is_off(emu)


def test_refusals_return_their_error_without_a_launch(emu):
    lref.check_refusals(emu)
