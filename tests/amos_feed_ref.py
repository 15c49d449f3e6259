"""Shared inputs and checks of the AMOS data-feed tests (tests/test_amos_feed_emu.py on the CPU emulator, tests/test_gpu_amos_feed.py on
the GPU; volume_feed_kernel in icl_amd/csrc/kernels/datafeed.h, icl_amd/dataloaders/amos.py).  Not a test module.

``forward_chain`` is the yardstick: a numpy restatement of the FORWARD chain of train_inherent_consistent_unet_3D_AMOS22.py:102-133 —
slice, ``np.pad``, ``np.flip``, ``np.rot90``, then two separate float32 operations for ``mul`` / ``add`` — deliberately the opposite
formulation from the kernel, which maps every output voxel backwards.  Every comparison is exact (``np.array_equal``, image and label):
one fp32 multiply and one fp32 add are the same IEEE operations on both sides.  MONAI is not installed, so this restates MONAI 1.0.1's
published definitions; parity with MONAI's own code is unpinned.

References are computed once per (sweep, ROI) and shared.
"""
import functools
import itertools

import numpy as np
import torch

from icl_amd.dataloaders.amos import OnDeviceAugmentAMOS
from icl_amd.dataloaders.brats2019 import DeviceVolumeStore
from icl_amd.utils.hashfill import hash_uniform_np

ROI_SCALAR = (6, 6, 5)      # R2 % 4 != 0: one thread per voxel
ROI_QUAD = (6, 6, 8)        # R2 % 4 == 0: one thread per four depth voxels when the outputs are 16-byte aligned
# against ROI_SCALAR: larger on every axis | axis 0 shorter (pad width 2), axis 2 equal (nothing padded, nothing drawn) |
# every axis shorter, odd pad widths 1, 3, 3 -> left pads 0, 1, 1
SOURCES = [(9, 7, 8), (4, 9, 5), (5, 3, 2)]
INTENSITIES = [(1.0, 0.0), (1.0, 0.0625), (1.25, -0.03125)]       # no shift | add | mul and add
BIG_ROI = (96, 96, 96)
BIG_SOURCES = [(130, 101, 70), (96, 96, 96), (97, 140, 96), (60, 200, 111)]


@functools.lru_cache(maxsize=None)
def source_volume(shape):
    """(image fp32, label uint8) filled with distinct values: the image 1.5, 2.0, 2.5, ... in memory order (never 0, exact in fp32),
    the label 1 + index % 255 (never 0, so a padded voxel cannot be mistaken for a source voxel)."""
    n = int(np.prod(shape))
    image = (1.5 + 0.5 * np.arange(n, dtype=np.float32)).reshape(shape)
    label = (1 + np.arange(n) % 255).astype(np.uint8).reshape(shape)
    return image, label


@functools.lru_cache(maxsize=None)
def big_volume(shape, seed):
    n = int(np.prod(shape))
    image = hash_uniform_np(n, seed, 1.0).reshape(shape)
    label = np.clip(((hash_uniform_np(n, seed + 1000, 0.5) + 0.5) * 16).astype(np.int64), 0, 15).astype(np.uint8).reshape(shape)
    return image, label


def make_row(shape, roi, origin, flip, k, mul=1.0, add=0.0):
    """One icl_volume_feed parameter row; ``origin[a]`` is used where the axis is larger than the ROI and must be 0 elsewhere."""
    size = [min(r, n) for r, n in zip(roi, shape)]
    assert all(0 <= o <= n - s for o, n, s in zip(origin, shape, size))
    left = [(r - s) // 2 for r, s in zip(roi, size)]
    return (*shape, *origin, *size, *left, flip, k, float(mul), float(add))


def forward_chain(image, label, row, roi):
    """(image [1, *roi] fp32, label [1, *roi] int64) of one sample, forwards."""
    c, s, left, flip, k = row[3:6], row[6:9], row[9:12], int(row[12]), int(row[13])
    mul, add = np.float32(row[14]), np.float32(row[15])
    window = tuple(slice(int(c[a]), int(c[a]) + int(s[a])) for a in range(3))
    widths = [(int(left[a]), roi[a] - int(s[a]) - int(left[a])) for a in range(3)]
    out = []
    for x in (image, label):
        x = np.pad(x[window], widths, mode="constant", constant_values=0)
        for a in range(3):
            if flip >> a & 1:
                x = np.flip(x, a)
        out.append(np.rot90(x, k, axes=(0, 1)))
    x = out[0].astype(np.float32)
    x = (x * mul).astype(np.float32)        # rounded ...
    x = (x + add).astype(np.float32)        # ... and rounded again
    return np.ascontiguousarray(x)[None], np.ascontiguousarray(out[1]).astype(np.int64)[None]


@functools.lru_cache(maxsize=None)
def sweep(roi):
    """Per source, all 8 flip masks x k = 0..3 x the three intensity settings, the source index fastest so that every launch of 16 mixes
    the sources; the crop origins walk through both ends of their range (and the middle).  Returns (indices, rows, want_image [N,1,*roi],
    want_label [N,1,*roi])."""
    indices, rows = [], []
    for m, ((mul, add), k, flip, src) in enumerate(itertools.product(INTENSITIES, range(4), range(8), range(len(SOURCES)))):
        shape = SOURCES[src]
        span = [max(n - r, 0) for n, r in zip(shape, roi)]
        pick = [(0, span[a], span[a] // 2)[(m // 3 + a + flip) % 3] for a in range(3)]
        indices.append(src)
        rows.append(make_row(shape, roi, pick, flip, k, mul, add))
    want = [forward_chain(*source_volume(SOURCES[i]), row, roi) for i, row in zip(indices, rows)]
    for src, shape in enumerate(SOURCES):      # both ends of every origin range are in the sweep
        for a in range(3):
            seen = {row[3 + a] for i, row in zip(indices, rows) if i == src}
            assert {0, max(shape[a] - roi[a], 0)} <= seen, (src, a, seen)
    return indices, rows, np.stack([w[0] for w in want]), np.stack([w[1] for w in want])


def small_store(device):
    return DeviceVolumeStore([source_volume(s) for s in SOURCES], device)


def check_sweep(store, roi, per_launch=16, misaligned_image=False):
    """The sweep in launches of ``per_launch`` mixed samples == the restatement, exactly.  ``misaligned_image``: the image output starts
    4 bytes past a 16-byte boundary (the launcher must then take the one-voxel-per-thread kernel)."""
    indices, rows, want_image, want_label = sweep(roi)
    feed = OnDeviceAugmentAMOS(store, roi)
    dev = store.device
    per = roi[0] * roi[1] * roi[2]
    for lo in range(0, len(indices), per_launch):
        idx, par = indices[lo:lo + per_launch], rows[lo:lo + per_launch]
        out = None
        if misaligned_image:
            buf = torch.full((len(idx) * per + 4,), float("nan"), dtype=torch.float32, device=dev)
            shift = 1 + (-(buf.data_ptr() // 4)) % 4                     # first element 4 bytes past a 16-byte boundary
            image = buf[shift:shift + len(idx) * per].view(len(idx), 1, *roi)
            assert image.data_ptr() % 16 == 4 and image.is_contiguous()
            out = (image, torch.full((len(idx), 1, *roi), -1, dtype=torch.int64, device=dev))
        got = feed.batch(idx, params=par, out=out)
        assert got["image"].shape == (len(idx), 1, *roi) and got["image"].dtype == torch.float32
        assert got["label"].shape == (len(idx), 1, *roi) and got["label"].dtype == torch.int64
        gi, gl = got["image"].cpu().numpy(), got["label"].cpu().numpy()
        for j in range(len(idx)):
            assert np.array_equal(gi[j], want_image[lo + j]), (roi, lo + j, par[j])
            assert np.array_equal(gl[j], want_label[lo + j]), (roi, lo + j, par[j])
    return len(indices)


def check_padded_voxels(store, roi):
    """Padded voxels hold exactly ``add`` (image; 0 * mul + add) and 0 (label); the others hold source values (never 0 here)."""
    src = 2                                                            # (5, 3, 2): padded on every axis
    shape = SOURCES[src]
    for flip, k, mul, add in ((0, 0, 1.0, 0.0625), (5, 3, 1.25, -0.03125), (7, 2, 1.0, 0.0)):
        row = make_row(shape, roi, (0, 0, 0), flip, k, mul, add)
        got = OnDeviceAugmentAMOS(store, roi).batch([src], params=[row])
        image, label = got["image"][0, 0].cpu().numpy(), got["label"][0, 0].cpu().numpy()
        padded = label == 0
        assert int((~padded).sum()) == int(np.prod(shape))             # every source voxel is in the patch, the rest is padding
        assert padded.sum() > 0 and (image[padded] == np.float32(add)).all()
        assert (image[~padded] != np.float32(add)).all()
        inside = np.zeros(roi, dtype=bool)                                # where the padding is, forwards
        left = row[9:12]
        inside[tuple(slice(left[a], left[a] + shape[a]) for a in range(3))] = True
        for a in range(3):
            if flip >> a & 1:
                inside = np.flip(inside, a)
        assert np.array_equal(~padded, np.rot90(inside, k, axes=(0, 1)))


def big_batch():
    """Four volumes -> 96^3 with explicit parameters: every flip bit and every k at least once, non-zero shifts, origins at the ends
    and inside their ranges; (96, 96, 96) crops nothing, (60, 200, 111) is padded on axis 0, (130, 101, 70) on axis 2."""
    rows = [make_row(BIG_SOURCES[0], BIG_ROI, (34, 0, 0), 0b001, 1, 1.0, 0.0625),
            make_row(BIG_SOURCES[1], BIG_ROI, (0, 0, 0), 0b110, 2, 1.125, -0.03125),
            make_row(BIG_SOURCES[2], BIG_ROI, (1, 44, 0), 0b100, 3, 1.0, 0.09375),
            make_row(BIG_SOURCES[3], BIG_ROI, (0, 57, 15), 0b011, 0, 0.9375, 0.015625)]
    assert {r[13] for r in rows} == {0, 1, 2, 3} and all(any(r[12] >> a & 1 for r in rows) for a in range(3))
    return [big_volume(s, 40 + i) for i, s in enumerate(BIG_SOURCES)], rows


@functools.lru_cache(maxsize=None)
def big_reference():
    volumes, rows = big_batch()
    want = [forward_chain(*v, row, BIG_ROI) for v, row in zip(volumes, rows)]
    return np.stack([w[0] for w in want]), np.stack([w[1] for w in want])


# ---- intensity: two roundings, told apart from one ----------------------------------------------------------------------------------

TWICE_SOURCES = [(9, 7, 8), (5, 3, 2)]                # larger than both small ROIs on every axis but the last | padded on every axis
TWICE_MUL, TWICE_ADD = np.float32(1.1), np.float32(0.07)
TWICE_DIFFERING = [146, 10]                           # voxels of each whole source at which one rounding and two give different fp32


@functools.lru_cache(maxsize=None)
def twice_volume(shape):
    """Hash-filled image (its products with 1.1 are inexact, unlike ``source_volume``'s) with ``source_volume``'s labels (never 0)."""
    return hash_uniform_np(int(np.prod(shape)), 7, 1.0).reshape(shape), source_volume(shape)[1]


def fused_intensity(x):
    """``x * mul + add`` rounded ONCE to fp32: what a contracted multiply-add would give."""
    return (x.astype(np.float64) * np.float64(TWICE_MUL) + np.float64(TWICE_ADD)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def twice_rows(roi):
    """16 samples, volume-major (8 of each source): all eight flip masks, k = 0..3 spread over them, origins walking their ranges.
    Returns (indices, rows, want_image, want_label) with ``forward_chain``'s values; asserts that a fused multiply-add would differ from
    them at one un-padded voxel or more of EVERY sample."""
    for shape, count in zip(TWICE_SOURCES, TWICE_DIFFERING):
        x = twice_volume(shape)[0]
        assert int((fused_intensity(x) != ((x * TWICE_MUL).astype(np.float32) + TWICE_ADD).astype(np.float32)).sum()) == count, shape
    indices, rows, want = [], [], []
    for src, shape in enumerate(TWICE_SOURCES):
        span = [max(n - r, 0) for n, r in zip(shape, roi)]
        for flip in range(8):
            origin = [(flip + a) % (span[a] + 1) for a in range(3)]
            row = make_row(shape, roi, origin, flip, (flip + src) % 4, TWICE_MUL, TWICE_ADD)
            image, label = twice_volume(shape)
            w = forward_chain(image, label, row, roi)
            plain, lab = forward_chain(image, label, (*row[:14], 1.0, 0.0), roi)       # the geometry alone
            source = lab != 0                                                          # the un-padded region
            assert (fused_intensity(plain)[source] != w[0][source]).any(), ("no voxel tells one rounding from two", shape, row)
            indices.append(src)
            rows.append(row)
            want.append(w)
    assert {r[12] for r in rows} == set(range(8)) and {r[13] for r in rows} == {0, 1, 2, 3}
    return indices, rows, np.stack([w[0] for w in want]), np.stack([w[1] for w in want])


def check_twice_rounded_intensity(device, roi):
    """``fp32(fp32(x * mul) + add)`` with values whose product is inexact (mul = 1.1, add = 0.07, hash-filled sources), so that a
    multiply-add contracted into one fma, in a kernel or in a helper it calls, gives other bits: the feed equals ``forward_chain``
    exactly through ``icl_volume_feed``, through ``icl_volume_feed_origins`` (``OnDeviceAugmentPosNeg``; every voxel is foreground, so
    rank = flat index of the crop's centre), and as the plain samples of an ``icl_volume_feed_affine`` launch; the affine samples of
    that launch equal ``affine_feed_ref.affine_chain``."""
    import affine_feed_ref as affine_ref
    from icl_amd.dataloaders.amos import KIND_FG, ForegroundIndex, OnDeviceAugmentPosNeg, affine_matrix
    indices, rows, want_image, want_label = twice_rows(roi)
    store = DeviceVolumeStore([twice_volume(s) for s in TWICE_SOURCES], device)

    def equal(got, what, expect=(want_image, want_label)):
        gi, gl = got["image"].cpu().numpy(), got["label"].cpu().numpy()
        for j, row in enumerate(rows):
            assert np.array_equal(gi[j], expect[0][j]), (what, "image", roi, j, row)
            assert np.array_equal(gl[j], expect[1][j]), (what, "label", roi, j, row)

    equal(OnDeviceAugmentAMOS(store, roi).batch(indices, params=rows), "volume_feed")

    posneg = []
    for row in rows:
        n, c, s = row[:3], row[3:6], row[6:9]
        centre = [c[a] + s[a] // 2 for a in range(3)]                                  # origin = clamp(centre - s // 2, 0, n - s) = c
        posneg.append((*n, 0, 0, 0, *row[6:16], KIND_FG, (centre[0] * n[1] + centre[1]) * n[2] + centre[2]))
    feed = OnDeviceAugmentPosNeg(store, ForegroundIndex(store), roi, num_samples=8)
    equal(feed.batch([0, 1], params=posneg), "volume_feed_origins")

    M = tuple(float(v) for v in affine_matrix((0.3, -0.2, 0.1), (1.1, 0.9, 1.0)).reshape(-1))
    with_affine = {3, 11}                                                              # one sample of each source
    mixed = [(*row, *M) if j in with_affine else row for j, row in enumerate(rows)]
    expect_image, expect_label = want_image.copy(), want_label.copy()
    for j in with_affine:
        expect_image[j], expect_label[j] = affine_ref.affine_chain(*twice_volume(TWICE_SOURCES[indices[j]]), rows[j], M, roi)
    equal(OnDeviceAugmentAMOS(store, roi).batch(indices, params=mixed), "volume_feed_affine", (expect_image, expect_label))
