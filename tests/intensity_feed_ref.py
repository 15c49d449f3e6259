"""Shared restatement and checks of the intensity stage of the 3-D feed (tests/test_intensity_feed_emu.py on the CPU emulator,
tests/test_gpu_intensity_feed.py on the GPU; icl_amd/csrc/kernels/intensity.h, icl_amd/dataloaders/intensity.py).  Not a test module.

The functions ``*_ref`` restate DESIGN.md §2 "Intensity stage of the 3-D feed" literally in numpy, one numpy operation per rounding the
definition names.  What is compared how:

* blur, statistics, contrast: EXACT (``np.array_equal``): the same IEEE operations on both sides, and the blur's restatement is itself
  bit-equal to ``scipy.ndimage.gaussian_filter`` (checked in the emulator's test file);
* noise and gamma go through ``log`` / ``cos`` / ``pow`` in double, whose last bit may differ between libraries.  A double result is
  rounded ONCE to fp32, so the two sides can differ only where the double sits within about 1e-16 (relative) of an fp32 rounding tie,
  and then by one fp32 ulp of that value.  Noise: ``|got - want| <= 2^-23 (|n| + |want|)`` on every voxel (an ulp of n is at most
  ``2^-23 |n|``, and the sum ``x + n`` is rounded once more: at most an ulp of the result on top).  Gamma: one fp32 ulp of
  ``max(|mn|, |mx|)``, the largest magnitude the result can have.  These follow from the formats, not from what the code gives; the
  number of voxels that differ at all is printed.

Inputs come from the project's counter hash, the same on every machine; references are computed once and shared.
"""
import functools

import numpy as np
import torch

from icl_amd.dataloaders.amos import ForegroundIndex, OnDeviceAugmentAMOS, OnDeviceAugmentPosNeg, draw_amos_params
from icl_amd.dataloaders.brats2019 import DeviceVolumeStore, OnDeviceAugment, draw_rotflip_crop
from icl_amd.dataloaders.intensity import (OFF_ROW, IntensityAugment, blur_radius, blur_weights, draw_intensity_params)
from icl_amd.utils.hashfill import hash_uniform_np
from icl_amd import _lib

SHAPE_SCALAR = (7, 9, 10)       # R2 % 4 != 0: the scalar paths
SHAPE_QUAD = (8, 12, 16)        # 16-byte paths; smallest extent 8 = the radius of sigma 2.0
SHAPE_CUBE = (16, 16, 16)
SHAPE_STATS = (32, 32, 32)      # 8192 quads: 32 workgroups of partial sums
SHAPE_BIG = (96, 96, 96)        # the trainer's patch: 64 workgroups, 13.5 quads a slot
SHAPE_ROUNDS = (40, 40, 44)     # 17,600 quads: the cap of 64 workgroups, and a second, partial quad for some slots only
SHAPES = [SHAPE_SCALAR, SHAPE_QUAD, SHAPE_CUBE, SHAPE_STATS, SHAPE_ROUNDS]
SCIPY_CASES = [((8, 12, 16), 2.0), ((7, 9, 10), 0.5), ((16, 16, 16), 1.0), ((32, 32, 32), 1.49), ((8, 8, 8), 1.87)]


def row(noise=None, blur=None, contrast=None, gamma=None):
    """An intensity row from what is on: ``noise=(seed, sigma, clip)``, ``blur=sigma``, ``contrast=f``, ``gamma=(g, invert)``."""
    r = list(OFF_ROW)
    if noise is not None:
        r[0:4] = [1, int(noise[0]), float(noise[1]), float(noise[2])]
    if blur is not None:
        r[4:6] = [1, float(blur)]
    if contrast is not None:
        r[6:8] = [1, float(np.float32(contrast))]
    if gamma is not None:
        r[8:11] = [1, float(gamma[0]), int(gamma[1])]
    return tuple(r)


@functools.lru_cache(maxsize=None)
def patch(shape, seed=7, lo=-0.75, hi=1.25):
    """A deterministic fp32 patch with values in [lo, hi)."""
    n = int(np.prod(shape))
    u = hash_uniform_np(n, seed, 0.5).astype(np.float64) + 0.5
    x = (lo + (hi - lo) * u).astype(np.float32).reshape(shape)
    x.setflags(write=False)
    return x


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------

def mix32_ref(x):
    x = x.astype(np.uint32, copy=True)
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7FEB352D)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846CA68B)
    x ^= x >> np.uint32(16)
    return x


def noise_values_ref(n_voxels, seed, sigma, clip):
    """n of every voxel of a sample, fp32: one pair of uniforms per voxel."""
    with np.errstate(over="ignore"):
        i = np.arange(n_voxels, dtype=np.uint32)
        h1 = mix32_ref(i * np.uint32(0x9E3779B1) + np.uint32(seed))
        h2 = mix32_ref(h1 + np.uint32(0x632BE5AB))
    u1 = (h1.astype(np.float64) + 0.5) / 4294967296.0
    u2 = h2.astype(np.float64) / 4294967296.0
    z = np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)
    n = (np.float64(sigma) * z).astype(np.float32)
    if clip > 0:
        limit = np.float32(np.float64(clip) * np.float64(sigma))
        n = np.minimum(np.maximum(n, -limit), limit)
    return n


def noise_ref(x, seed, sigma, clip):
    n = noise_values_ref(x.size, seed, sigma, clip).reshape(x.shape)
    return (x + n).astype(np.float32), n


def blur_weights_ref(sigma):
    r = int(4.0 * sigma + 0.5)
    k = np.arange(0, r + 1, dtype=np.float64)
    full = np.exp(-0.5 / (sigma * sigma) * np.arange(-r, r + 1) ** 2)       # scipy's _gaussian_kernel1d: exponent argument and all
    return (full / full.sum())[r:], r, k


def blur_ref(x, sigma):
    """Axes 0, 1, 2 in turn; per output, in double, acc = w_0 x[c], then acc = acc + (x[c - k] + x[c + k]) w_k, one rounding to fp32."""
    w, r, _ = blur_weights_ref(float(sigma))
    x = np.asarray(x, dtype=np.float32)
    for axis in range(3):
        n = x.shape[axis]
        assert r <= n
        pad = [(0, 0)] * 3
        pad[axis] = (r, r)
        xp = np.pad(x.astype(np.float64), pad, mode="symmetric")              # d c b a | a b c d | d c b a
        take = lambda lo: np.take(xp, np.arange(lo, lo + n), axis=axis)       # noqa: E731
        acc = w[0] * take(r)
        for k in range(1, r + 1):
            acc = acc + (take(r - k) + take(r + k)) * w[k]
        x = acc.astype(np.float32)
    return x


def stat_blocks(n_voxels):
    return min(64, max(1, -(-(-(-n_voxels // 4)) // 256)))


def stats_ref(x):
    """(min, max, mean) fp32 with the sum in the kernels' fixed order: voxel i belongs to slot (i // 4) % (256 G); a slot adds its voxels
    in increasing i; the 256 slots of a workgroup are halved with t += t + d, d = 128 .. 1; the G workgroup sums are added in order."""
    v = np.asarray(x, dtype=np.float32).reshape(-1)
    n = v.size
    g = stat_blocks(n)
    slots = 256 * g
    rounds = -(-n // (4 * slots))
    padded = np.zeros(rounds * slots * 4, dtype=np.float64)                   # + 0.0 changes no double that started at 0.0
    padded[:n] = v
    padded = padded.reshape(rounds, slots, 4)
    acc = np.zeros(slots, dtype=np.float64)
    for it in range(rounds):
        for t in range(4):
            acc = acc + padded[it, :, t]
    acc = acc.reshape(g, 256)
    d = 128
    while d >= 1:
        acc = acc[:, :d] + acc[:, d:2 * d]
        d //= 2
    total = np.float64(0.0)
    for b in range(g):
        total = acc[b, 0] if b == 0 else total + acc[b, 0]
    return np.float32(v.min()), np.float32(v.max()), np.float32(total / np.float64(n))


def contrast_ref(x, f, mn, mx, mean):
    f, mn, mx, mean = np.float32(f), np.float32(mn), np.float32(mx), np.float32(mean)
    d = (np.asarray(x, dtype=np.float32) - mean).astype(np.float32)
    d = (d * f).astype(np.float32)
    d = (d + mean).astype(np.float32)
    return np.minimum(np.maximum(d, mn), mx).astype(np.float32)


def gamma_ref(x, g, invert, lo, hi):
    """``lo`` / ``hi``: the extremes of the input (after contrast), fp32.  Returns (y fp32, the magnitude the bound refers to)."""
    lo, hi = np.float32(lo), np.float32(hi)
    if invert:
        lo, hi = np.float32(-hi), np.float32(-lo)
    v = -np.asarray(x, dtype=np.float32) if invert else np.asarray(x, dtype=np.float32)
    dlo = np.float64(lo)
    rng = np.float64(hi) - np.float64(lo)
    den = rng + 1e-7
    t = (v.astype(np.float64) - dlo) / den
    p = t if g == 1.0 else np.power(t, np.float64(g))
    a = (p * rng).astype(np.float32)
    y = (a.astype(np.float64) + dlo).astype(np.float32)
    return (-y if invert else y), max(abs(float(lo)), abs(float(hi)))


def point_ref(x, r, stats):
    """Contrast and gamma of one sample from GIVEN statistics (min, max, mean): (y, gamma's magnitude or None)."""
    mn, mx, mean = (np.float32(v) for v in stats[:3])
    lo, hi = mn, mx
    if r[6]:
        x = contrast_ref(x, r[7], mn, mx, mean)
        lo, hi = contrast_ref(np.array([mn, mx], dtype=np.float32), r[7], mn, mx, mean)
    mag = None
    if r[8]:
        x, mag = gamma_ref(x, r[9], r[10], lo, hi)
    return x, mag


def chain_ref(x, r):
    """The whole stage on one sample with the restatement's own statistics: (y fp32, stats or None, per-voxel slack)."""
    x = np.asarray(x, dtype=np.float32)
    slack = np.zeros(x.shape, dtype=np.float64)
    if r[0]:
        x, n = noise_ref(x, r[1], r[2], r[3])
        slack = 2.0 ** -23 * (np.abs(n).astype(np.float64) + np.abs(x))
    if r[4]:
        x = blur_ref(x, r[5])
    stats = None
    if r[6] or r[8]:
        stats = stats_ref(x)
        x, mag = point_ref(x, r, stats)
        if mag is not None:
            slack = np.full(x.shape, float(np.spacing(np.float32(mag))), dtype=np.float64)
    return x, stats, slack


# ---- running the stage ------------------------------------------------------------------------------------------------------------------

def run_stage(device, samples, rows, misaligned=False):
    """``IntensityAugment.apply`` on a batch built from ``samples`` (same shape): (result [B, *shape] numpy, stats [B, 4] numpy)."""
    shape = samples[0].shape
    n, per = len(samples), int(np.prod(shape))
    stage = IntensityAugment(shape)
    if misaligned:
        buf = torch.zeros(n * per + 4, dtype=torch.float32, device=device)
        shift = 1 + (-(buf.data_ptr() // 4)) % 4
        image = buf[shift:shift + n * per].view(n, 1, *shape)
        assert image.data_ptr() % 16 == 4
    else:
        image = torch.empty((n, 1, *shape), dtype=torch.float32, device=device)
    image.copy_(torch.as_tensor(np.stack(samples)[:, None]))
    out = stage.apply(image, rows)
    assert out.data_ptr() == image.data_ptr()
    return out.cpu().numpy()[:, 0], stage.stats.cpu().numpy()


def differing(got, want):
    return int((got.view(np.uint32) != want.view(np.uint32)).sum())


# ---- the checks, shared by the emulator and the GPU -----------------------------------------------------------------------------------------

def check_blur(device):
    """Bit-equal to the restatement: r equal to the smallest extent, r = 0 (identity), several sigmas in one launch, both paths."""
    total = 0
    for shape, sigmas in ((SHAPE_QUAD, (2.0, 0.1, 0.5, 1.3)), (SHAPE_SCALAR, (0.5, 1.0, 1.6, 0.1)), (SHAPE_CUBE, (1.0, 2.9, 0.7)),
                          (SHAPE_STATS, (1.49,))):
        for misaligned in (False, True):
            samples = [patch(shape, 11 + j) for j in range(len(sigmas))] + [patch(shape, 3)]
            rows = [row(blur=s) for s in sigmas] + [row()]
            got, _ = run_stage(device, samples, rows, misaligned)
            for j, s in enumerate(sigmas):
                want = samples[j] if blur_radius(s) == 0 else blur_ref(samples[j], s)
                assert np.array_equal(got[j].view(np.uint32), want.view(np.uint32)), (shape, s, misaligned)
                total += 1
            assert np.array_equal(got[-1].view(np.uint32), samples[-1].view(np.uint32)), "a sample without the blur changed"
    assert blur_radius(2.0) == min(SHAPE_QUAD) and blur_radius(0.1) == 0 and blur_radius(2.9) == 12
    return total


def contrast_cases(shape):
    base = patch(shape, 21)
    const = np.full(shape, np.float32(0.3125), dtype=np.float32)
    return [(base, 0.75), (base, 1.25), (patch(shape, 22, 10.0, 11.0), 1.2000000476837158), (const, 1.1), (patch(shape, 23), 0.9)]


def check_contrast(device, shape):
    cases = contrast_cases(shape)
    samples = [c[0] for c in cases]
    rows = [row(contrast=c[1]) for c in cases]
    got, stats = run_stage(device, samples, rows)
    clipped = 0
    for j, (x, f) in enumerate(cases):
        mn, mx, mean = stats_ref(x)
        assert stats[j, 0] == x.min() and stats[j, 1] == x.max(), (shape, j)
        assert np.float32(stats[j, 2]).view(np.uint32) == mean.view(np.uint32), (shape, j, stats[j, 2], mean)
        exact = x.astype(np.float64).mean()
        bound = 2.0 ** -23 * float(np.abs(x).max())
        print(f"{shape} case {j}: mean {stats[j, 2]!r}, |mean - float64 mean| {abs(float(stats[j, 2]) - exact):.3e} (bound {bound:.3e})")
        assert abs(float(stats[j, 2]) - exact) <= bound
        assert stats[j, 3] == 0
        want, _ = point_ref(x, rows[j], stats[j])                              # the device's own statistics
        assert np.array_equal(got[j].view(np.uint32), want.view(np.uint32)), (shape, j)
        unclipped = ((x - stats[j, 2]).astype(np.float32) * np.float32(f)).astype(np.float32) + stats[j, 2]
        clipped += int(((unclipped < x.min()) | (unclipped > x.max())).sum())
        assert got[j].min() >= x.min() and got[j].max() <= x.max()
    assert clipped > 0, "no case with an active clip"
    assert np.array_equal(got[3], cases[3][0]), "a constant patch must stay as it is"
    return len(cases)


def check_noise(device, shape):
    x = patch(shape, 31)
    rows = [row(noise=(12345, 0.1, 0.0)), row(noise=(12345, 0.1, 0.0)), row(noise=(54321, 0.1, 0.0)), row(noise=(4294967295, 0.05, 2.0)), row()]
    got, _ = run_stage(device, [x] * len(rows), rows)
    assert np.array_equal(got[0].view(np.uint32), got[1].view(np.uint32)), "the same seed must repeat bit for bit"
    assert differing(got[0], got[2]) > x.size // 2, "another seed must give another field"
    assert np.array_equal(got[4].view(np.uint32), x.view(np.uint32))
    for j in (0, 2, 3):
        want, n = noise_ref(x, *rows[j][1:4])
        diff = np.abs(got[j].astype(np.float64) - want.astype(np.float64))
        bound = 2.0 ** -23 * (np.abs(n).astype(np.float64) + np.abs(want).astype(np.float64))
        print(f"noise {shape} row {j}: {differing(got[j], want)} of {x.size} voxels differ at all, worst |diff| {diff.max():.3e}")
        assert (diff <= bound).all(), (shape, j, float((diff - bound).max()))
    limit = np.float32(2.0 * 0.05)
    assert np.abs((got[3].astype(np.float64) - x.astype(np.float64))).max() <= float(limit) + 2.0 ** -23 * 2.0
    return 3


def check_gamma(device, shape):
    x = patch(shape, 41)
    cases = [(0.7, 0), (1.5, 0), (0.85, 1), (1.3, 1), (1.0, 0), (1.0, 1)]
    rows = [row(gamma=c) for c in cases] + [row(contrast=1.25, gamma=(1.4, 0)), row(contrast=0.8, gamma=(0.75, 1))]
    got, stats = run_stage(device, [x] * len(rows), rows)
    for j, r in enumerate(rows):
        assert stats[j, 0] == x.min() and stats[j, 1] == x.max()
        want, mag = point_ref(x, r, stats[j])
        diff = np.abs(got[j].astype(np.float64) - want.astype(np.float64))
        ulp = float(np.spacing(np.float32(mag)))
        print(f"gamma {shape} row {j} (g {r[9]}, invert {r[10]}, contrast {r[6]}): {differing(got[j], want)} of {x.size} voxels differ at all, "
              f"worst |diff| {diff.max():.3e} (one ulp {ulp:.3e})")
        assert (diff <= ulp).all(), (shape, j)
        if r[9] == 1.0:                                                       # pow(t, 1) is t: nothing inexact is left
            assert np.array_equal(got[j].view(np.uint32), want.view(np.uint32)), (shape, j)
            rng = np.float64(x.max()) - np.float64(x.min())
            v = -x if r[10] else x
            lo = np.float64(-x.max() if r[10] else x.min())
            t = (v.astype(np.float64) - lo) / (rng + 1e-7)
            y = ((t * rng).astype(np.float32).astype(np.float64) + lo).astype(np.float32)
            assert np.array_equal(got[j], -y if r[10] else y)
    return len(rows)


def check_noise_distribution(device):
    """Independent of the restatement: 32^3 voxels, sigma 0.1, on a zero patch (x + n = n exactly): the sample mean, the sample variance
    and the share beyond 2 sigma within five standard errors of 0, sigma^2 and 0.0455; with clip = 2 nothing beyond 2 sigma."""
    shape, sigma = SHAPE_STATS, 0.1
    zero = np.zeros(shape, dtype=np.float32)
    got, _ = run_stage(device, [zero, zero], [row(noise=(2024, sigma, 0.0)), row(noise=(2024, sigma, 2.0))])
    n = got[0].astype(np.float64).reshape(-1)
    count = n.size
    mean, var = n.mean(), n.var()
    tail = float((np.abs(n) > 2 * sigma).mean())
    p = 0.04550026389635842                                                   # 2 (1 - Phi(2))
    se_mean, se_var, se_tail = sigma / np.sqrt(count), sigma ** 2 * np.sqrt(2.0 / count), np.sqrt(p * (1 - p) / count)
    print(f"noise distribution: mean {mean:.3e} (se {se_mean:.3e}), variance {var:.6e} (expected {sigma ** 2:.6e}, se {se_var:.3e}), "
          f"share beyond 2 sigma {tail:.5f} (expected {p:.5f}, se {se_tail:.5f})")
    assert abs(mean) <= 5 * se_mean and abs(var - sigma ** 2) <= 5 * se_var and abs(tail - p) <= 5 * se_tail
    assert np.abs(got[1]).max() <= np.float32(2.0 * sigma)
    assert int((np.abs(got[1]) == np.float32(2.0 * sigma)).sum()) > 0


# ---- the loaders -------------------------------------------------------------------------------------------------------------------------

STORE_SHAPES = [(13, 17, 19), (9, 12, 16), (20, 9, 11)]
CHAIN_ROI = (8, 8, 12)


@functools.lru_cache(maxsize=None)
def store_volumes():
    out = []
    for j, s in enumerate(STORE_SHAPES):
        n = int(np.prod(s))
        image = hash_uniform_np(n, 60 + j, 1.0).reshape(s)
        label = (1 + np.arange(n) % 7).astype(np.uint8).reshape(s)
        label[hash_uniform_np(n, 70 + j, 1.0).reshape(s) < 0] = 0
        out.append((image, label))
    return out


def loader_store(device):
    return DeviceVolumeStore(store_volumes(), device)


ALL_ON = dict(noise_prob=1.0, noise_sigma=(0.02, 0.1), noise_clip=2.0, blur_prob=1.0, blur_sigma=(0.5, 1.5), contrast_prob=1.0,
              gamma_prob=1.0, invert_prob=0.5)


def chain_rows():
    """17 rows: every transform on in most, each transform alone, nothing, and pairs."""
    rows = draw_intensity_params(np.random.RandomState(5), 9, **ALL_ON)
    rows += [row(noise=(77, 0.1, 0.0)), row(blur=1.2), row(contrast=0.8), row(gamma=(1.3, 1)), row(), row(blur=0.6, contrast=1.25),
             row(contrast=1.1, gamma=(0.8, 0)), row(blur=2.0, gamma=(1.0, 1))]
    assert len(rows) == 17 and all(sum(r[k] for k in (0, 4, 6, 8)) == 4 for r in rows[:9])
    return rows


def compare_with_chain(plain, got, rows, what):
    """``got`` == the restatement applied to the plain feed's output: exact for a sample without noise and gamma, else within the slack."""
    slack_used = 0
    for j, r in enumerate(rows):
        want, _, slack = chain_ref(plain[j], r)
        if not (r[0] or r[8]):
            assert np.array_equal(got[j].view(np.uint32), want.view(np.uint32)), (what, j, r)
        else:
            diff = np.abs(got[j].astype(np.float64) - want.astype(np.float64))
            assert (diff <= slack).all(), (what, j, r, float(diff.max()))
            slack_used += differing(got[j], want)
    print(f"{what}: {slack_used} voxels differ at all over {len(rows)} samples")


def check_chain_amos(device):
    """One batch of 17 through OnDeviceAugmentAMOS(intensity=...): two chunks, equal to the restatement on the plain feed's output, labels
    untouched, and bit for bit the same when run again with the same rows."""
    store = loader_store(device)
    indices = [j % len(STORE_SHAPES) for j in range(17)]
    geo = OnDeviceAugmentAMOS(store, CHAIN_ROI, rng=np.random.RandomState(3), flip_prob=0.5, rot_prob=0.0).draw(indices)
    plain = OnDeviceAugmentAMOS(store, CHAIN_ROI, rot_prob=0.0).batch(indices, params=geo)
    feed = OnDeviceAugmentAMOS(store, CHAIN_ROI, rot_prob=0.0, intensity=IntensityAugment(CHAIN_ROI, **ALL_ON))
    rows = chain_rows()
    got = feed.batch(indices, params=geo, intensity_params=rows)
    assert torch.equal(got["label"], plain["label"])
    first = got["image"].cpu().numpy()[:, 0]
    compare_with_chain(plain["image"].cpu().numpy()[:, 0], first, rows, "AMOS feed")
    again = feed.batch(indices, params=geo, intensity_params=rows)["image"].cpu().numpy()[:, 0]
    assert np.array_equal(first.view(np.uint32), again.view(np.uint32))
    assert tuple(feed.intensity.stats.shape) == (17, 4)


def check_chain_other_stores(device):
    """The BraTS feed and the pos/neg feed with the stage: the restatement applied to their plain output."""
    store = loader_store(device)
    patch_size = (8, 8, 8)
    np.random.seed(9)
    geo = [draw_rotflip_crop(store.images[i].shape, patch_size) for i in (0, 1, 2)]
    rows = chain_rows()[:2] + [row(blur=1.0, contrast=0.9)]
    plain = OnDeviceAugment(store, patch_size).batch([0, 1, 2], params=geo)
    got = OnDeviceAugment(store, patch_size, intensity=IntensityAugment(patch_size, **ALL_ON)).batch([0, 1, 2], params=geo, intensity_params=rows)
    assert torch.equal(got["label"], plain["label"]) and got["image"].shape == (3, 1, *patch_size)
    compare_with_chain(plain["image"].cpu().numpy()[:, 0], got["image"].cpu().numpy()[:, 0], rows, "BraTS feed")
    index = ForegroundIndex(store)
    kw = dict(num_samples=2, rot_prob=0.0)
    geo = OnDeviceAugmentPosNeg(store, index, CHAIN_ROI, rng=np.random.RandomState(4), **kw).draw([2, 0])
    rows = chain_rows()[7:11]
    plain = OnDeviceAugmentPosNeg(store, index, CHAIN_ROI, **kw).batch([2, 0], params=geo)
    got = OnDeviceAugmentPosNeg(store, index, CHAIN_ROI, intensity=IntensityAugment(CHAIN_ROI, **ALL_ON), **kw).batch(
        [2, 0], params=geo, intensity_params=rows)
    assert torch.equal(got["label"], plain["label"]) and got["image"].shape == (4, 1, *CHAIN_ROI)
    compare_with_chain(plain["image"].cpu().numpy()[:, 0], got["image"].cpu().numpy()[:, 0], rows, "pos/neg feed")


def check_off_is_off(device):
    """intensity=None and a stage whose probabilities are all 0: the same batches from the same seed, the generator left in the same
    state; a mixed batch leaves the samples that drew nothing as the plain feed gives them."""
    store = loader_store(device)
    indices = [0, 1, 2, 1]
    a, b = np.random.RandomState(17), np.random.RandomState(17)
    plain = OnDeviceAugmentAMOS(store, CHAIN_ROI, rng=a, rot_prob=0.0).batch(indices)
    stage = IntensityAugment(CHAIN_ROI, rng=b, noise_prob=0.0, blur_prob=0, contrast_prob=0.0, gamma_prob=0.0, invert_prob=0.7,
                             noise_sigma=(0.1, 0.2), blur_sigma=1.0)
    assert not stage.enabled
    off = OnDeviceAugmentAMOS(store, CHAIN_ROI, rng=b, rot_prob=0.0, intensity=stage).batch(indices)
    assert torch.equal(plain["image"], off["image"]) and torch.equal(plain["label"], off["label"])
    assert a.rand() == b.rand()
    index = ForegroundIndex(store)
    a, b = np.random.RandomState(18), np.random.RandomState(18)
    plain_pn = OnDeviceAugmentPosNeg(store, index, CHAIN_ROI, num_samples=2, rng=a, rot_prob=0.0).batch([0, 2])
    off_pn = OnDeviceAugmentPosNeg(store, index, CHAIN_ROI, num_samples=2, rng=b, rot_prob=0.0,
                                   intensity=IntensityAugment(CHAIN_ROI, rng=b)).batch([0, 2])
    assert torch.equal(plain_pn["image"], off_pn["image"]) and a.rand() == b.rand()
    np.random.seed(19)
    plain_b = OnDeviceAugment(store, (8, 8, 8)).batch([0, 1])
    state = np.random.get_state()[1].copy()
    np.random.seed(19)
    off_b = OnDeviceAugment(store, (8, 8, 8), intensity=IntensityAugment((8, 8, 8))).batch([0, 1])
    assert torch.equal(plain_b["image"], off_b["image"]) and np.array_equal(state, np.random.get_state()[1])
    # mixed: samples 1 and 3 drew nothing
    geo = OnDeviceAugmentAMOS(store, CHAIN_ROI, rng=np.random.RandomState(2), rot_prob=0.0).draw(indices)
    base = OnDeviceAugmentAMOS(store, CHAIN_ROI, rot_prob=0.0).batch(indices, params=geo)["image"].cpu().numpy()
    rows = [row(blur=1.0, gamma=(1.2, 0)), row(), row(noise=(1, 0.1, 2.0), contrast=1.2), row()]
    mixed = OnDeviceAugmentAMOS(store, CHAIN_ROI, rot_prob=0.0, intensity=IntensityAugment(CHAIN_ROI)).batch(
        indices, params=geo, intensity_params=rows)["image"].cpu().numpy()
    for j in (1, 3):
        assert np.array_equal(mixed[j].view(np.uint32), base[j].view(np.uint32))
    for j in (0, 2):
        assert differing(mixed[j], base[j]) > 0


def check_refusals(device):
    """Every refusal of the four entry points returns -1 with its message and writes nothing (the batch is compared afterwards)."""
    import ctypes
    L = _lib.lib()
    shape = (8, 12, 16)
    per = int(np.prod(shape))
    x = torch.as_tensor(np.stack([patch(shape, 51), patch(shape, 52)])).to(device).contiguous()
    before = x.clone()
    scratch = torch.zeros_like(x)
    stats = torch.zeros((2, 4), dtype=torch.float32, device=device)
    ws = torch.zeros(16 * 64 * 3, dtype=torch.float64, device=device)
    D = lambda *v: (ctypes.c_double * len(v))(*v)                             # noqa: E731
    nan, inf = float("nan"), float("inf")

    def refused(rc, text):
        assert rc == -1, (rc, text)
        msg = L.icl_last_error().decode()
        assert text in msg, (text, msg)

    ok_noise = (1.0, 5.0, 0.1, 0.0)
    noise = lambda p, b=2, ptr=x.data_ptr(), r=shape: L.icl_intensity_noise(ptr, p, b, *r, None)        # noqa: E731
    refused(noise(None), "null pointer")
    refused(noise(D(*ok_noise * 2), ptr=None), "null pointer")
    refused(noise(D(*ok_noise * 2), b=0), "batch")
    refused(noise(D(*ok_noise * 2), b=17), "batch")
    refused(noise(D(*ok_noise * 2), r=(0, 12, 16)), "extents")
    refused(noise(D(*ok_noise * 2), r=(2048, 2048, 1024)), "2^31")
    for bad, text in (((2.0, 5.0, 0.1, 0.0), "flag"), ((0.5, 5.0, 0.1, 0.0), "flag"), ((1.0, -1.0, 0.1, 0.0), "seed"),
                      ((1.0, 4294967296.0, 0.1, 0.0), "seed"), ((1.0, 0.5, 0.1, 0.0), "seed"), ((1.0, 5.0, 0.0, 0.0), "sigma"),
                      ((1.0, 5.0, -0.1, 0.0), "sigma"), ((0.0, 5.0, nan, 0.0), "sigma"), ((1.0, 5.0, inf, 0.0), "sigma"),
                      ((1.0, 5.0, 0.1, -1.0), "clip"), ((1.0, 5.0, 0.1, nan), "clip")):
        refused(noise(D(*ok_noise, *bad)), text)

    w = [float(v) for v in blur_weights(1.0)]
    ok_blur = (1.0, 1.0, *w, *([0.0] * (13 - len(w))))
    blur = lambda p, b=2, ptr=x.data_ptr(), sc=scratch.data_ptr(), r=shape: L.icl_intensity_blur(ptr, sc, p, b, *r, None)   # noqa: E731
    refused(blur(None), "null pointer")
    refused(blur(D(*ok_blur * 2), sc=None), "null pointer")
    refused(blur(D(*ok_blur * 2), ptr=None), "null pointer")
    refused(blur(D(*ok_blur * 2), sc=x.data_ptr()), "scratch")
    refused(blur(D(*ok_blur * 2), b=17), "batch")
    refused(blur(D(*ok_blur * 2), r=(1, 1, 4097)), "contiguous axis")
    refused(blur(D(*ok_blur * 2), r=(65536, 65536, 1)), "2^31")
    w3 = [float(v) for v in blur_weights(3.0)]
    for bad, text in (((1.0, 0.0, *w, *([0.0] * 8)), "sigma"), ((1.0, -1.0, *w, *([0.0] * 8)), "sigma"), ((0.0, nan, *w, *([0.0] * 8)), "sigma"),
                      ((1.0, inf, *w, *([0.0] * 8)), "sigma"), ((1.0, 3.2, *w3), "radius 13"), ((1.0, 1e300, *w3), "at most 12"),
                      ((1.0, 2.2, *w3), "smallest extent"), ((3.0, 1.0, *w, *([0.0] * 8)), "flag"),
                      ((1.0, 1.0, nan, *w[1:], *([0.0] * 8)), "weight"), ((1.0, 1.0, w[0], 1.5, *w[2:], *([0.0] * 8)), "weight")):
        assert len(bad) == 15
        refused(blur(D(*ok_blur, *bad)), text)

    I = lambda *v: (ctypes.c_int32 * len(v))(*v)                               # noqa: E731
    st = lambda f, b=2, ptr=x.data_ptr(), s=stats.data_ptr(), w_=ws.data_ptr(), r=shape: L.icl_intensity_stats(ptr, f, b, *r, s, w_, None)   # noqa: E731
    refused(st(None), "null pointer")
    refused(st(I(1, 1), s=None), "null pointer")
    refused(st(I(1, 1), w_=None), "null pointer")
    refused(st(I(1, 1), ptr=None), "null pointer")
    refused(st(I(1, 2)), "flag")
    refused(st(I(-1, 1)), "flag")
    refused(st(I(1, 1), b=0), "batch")
    refused(st(I(1, 1), r=(8, -1, 16)), "extents")

    ok_point = (1.0, 1.1, 1.0, 1.2, 0.0)
    pt = lambda p, b=2, ptr=x.data_ptr(), s=stats.data_ptr(), r=shape: L.icl_intensity_point(ptr, s, p, b, *r, None)   # noqa: E731
    refused(pt(None), "null pointer")
    refused(pt(D(*ok_point * 2), s=None), "null pointer")
    refused(pt(D(*ok_point * 2), ptr=None), "null pointer")
    refused(pt(D(*ok_point * 2), b=17), "batch")
    refused(pt(D(*ok_point * 2), r=(2048, 2048, 1024)), "2^31")
    for bad, text in (((2.0, 1.1, 1.0, 1.2, 0.0), "contrast flag"), ((1.0, 1.1, -1.0, 1.2, 0.0), "gamma flag"), ((1.0, 1.1, 1.0, 1.2, 0.5), "invert flag"),
                      ((1.0, 0.0, 1.0, 1.2, 0.0), "contrast factor"), ((0.0, -1.0, 0.0, 1.2, 0.0), "contrast factor"), ((1.0, nan, 1.0, 1.2, 0.0), "contrast factor"),
                      ((1.0, inf, 1.0, 1.2, 0.0), "contrast factor"), ((1.0, 1e-60, 1.0, 1.2, 0.0), "contrast factor"), ((1.0, 1e60, 1.0, 1.2, 0.0), "contrast factor"),
                      ((1.0, 1.1, 1.0, 0.0, 0.0), "gamma"), ((1.0, 1.1, 0.0, -2.0, 0.0), "gamma"), ((1.0, 1.1, 1.0, nan, 0.0), "gamma"),
                      ((1.0, 1.1, 1.0, inf, 0.0), "gamma")):
        refused(pt(D(*ok_point, *bad)), text)
    assert torch.equal(x, before) and not scratch.any() and not stats.any() and not ws.any()
    assert per == x[0].numel()
