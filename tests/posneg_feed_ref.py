"""Shared inputs and checks of the pos/neg data-feed tests (tests/test_posneg_feed_emu.py on the CPU emulator, tests/test_gpu_posneg_feed.py
on the GPU; rank_count_kernel / rank_scan_kernel / rank_select_kernel in icl_amd/csrc/kernels/rankindex.h, volume_feed_kernel<V, true> in
datafeed.h, icl_amd/dataloaders/amos.py).  Not a test module.

The yardstick is numpy: ``flatnonzero`` of the two masks, ``unravel_index``, the clamp of ``correct_crop_centers`` + ``SpatialCrop``, and
``amos_feed_ref.forward_chain`` on the crop so found.  Every comparison is exact.  MONAI is not installed, so this restates MONAI 1.0.1's
published definitions of ``RandCropByPosNegLabeld``; parity with MONAI's own code is unpinned.

The shapes are chosen for kRankTile = 1024: less than one tile, exactly one tile, four tiles and a partial one, a constructed volume with
two whole tiles of nothing but background between foreground voxels (and a whole tile without background), and a volume smaller than
the ROI on every axis.  References are computed once and shared.
"""
import functools

import numpy as np
import torch

import amos_feed_ref as aref
from icl_amd import _lib
from icl_amd.dataloaders.amos import KIND_BG, KIND_FG, ForegroundIndex, OnDeviceAugmentPosNeg
from icl_amd.dataloaders.brats2019 import DeviceVolumeStore
from icl_amd.utils.hashfill import hash_uniform_np

TILE = 1024
ROI_SCALAR = aref.ROI_SCALAR          # (6, 6, 5): one thread per voxel
ROI_QUAD = aref.ROI_QUAD              # (6, 6, 8): one thread per four depth voxels
GAP_SHAPE = (12, 16, 24)              # 4,608 voxels: four tiles and a half
SHAPES = [(7, 9, 11), (8, 16, 8), (13, 17, 19), GAP_SHAPE, (5, 3, 2)]
THRESHOLD = 0.0


@functools.lru_cache(maxsize=None)
def volume(v):
    """(image fp32, label uint8) of SHAPES[v].  Hash-filled: about a third foreground, the image in [-1, 1] (about half the background
    above the threshold), one NaN on a background voxel and one on a foreground voxel.  GAP_SHAPE is constructed: foreground up to the
    LAST voxel of tile 0, tiles 1 and 2 nothing but background above the threshold, foreground again from the FIRST voxel of tile 3,
    tile 3 without any background (image <= threshold wherever the label is 0), background again in the partial tile 4."""
    shape = SHAPES[v]
    n = int(np.prod(shape))
    image = hash_uniform_np(n, 70 + v, 1.0).astype(np.float32)
    label = np.where(hash_uniform_np(n, 80 + v, 1.0) > 0.33, 1 + np.arange(n) % 7, 0).astype(np.uint8)
    if shape == GAP_SHAPE:
        label[TILE:3 * TILE] = 0
        image[TILE:3 * TILE] = 0.25 + 0.5 * np.abs(image[TILE:3 * TILE])
        label[TILE - 1] = 3
        label[3 * TILE] = 5
        stretch = slice(3 * TILE, 4 * TILE)
        image[stretch] = np.where(label[stretch] == 0, -np.abs(image[stretch]), image[stretch])
        image[3 * TILE + 7] = 0.0                                  # == threshold: not above it
        label[3 * TILE + 7] = 0
    zeros, ones = np.flatnonzero(label == 0), np.flatnonzero(label != 0)
    if shape != GAP_SHAPE and len(zeros) and len(ones):
        image[zeros[len(zeros) // 2]] = np.nan
        image[ones[len(ones) // 2]] = np.nan
    return image.reshape(shape), label.reshape(shape)


def lists(image, label, threshold=THRESHOLD):
    """(fg_idx, bg_idx): positions in the C-order ravel."""
    with np.errstate(invalid="ignore"):
        above = image > threshold                                  # NaN > t is False
    return np.flatnonzero(label != 0), np.flatnonzero(above & (label == 0))


def index_reference(image, label, threshold=THRESHOLD, tile=TILE):
    """The two prefix arrays: per-tile member counts, cumulated, with a leading 0."""
    n = image.size
    tiles = -(-n // tile)
    out = []
    for idx in lists(image, label, threshold):
        counts = np.bincount(idx // tile, minlength=tiles)
        out.append(np.concatenate([[0], np.cumsum(counts)]).astype(np.int64))
    return out


def origin_reference(shape, roi, flat):
    centre = np.unravel_index(int(flat), shape)
    size = [min(r, n) for r, n in zip(roi, shape)]
    return [int(min(max(int(c) - s // 2, 0), n - s)) for c, s, n in zip(centre, size, shape)]


def make_row(shape, roi, kind, rank, flip=0, k=0, mul=1.0, add=0.0):
    """One draw_posneg_params row: the 16 feed values with unused origin fields, then (kind, rank)."""
    return (*aref.make_row(shape, roi, (0, 0, 0), flip, k, mul, add), kind, rank)


def feed_row(v, row, roi):
    """The icl_volume_feed row the reference crops with: the origin found through numpy's lists."""
    image, label = volume(v) if isinstance(v, int) else v
    idx = lists(image, label)[int(row[16])]
    origin = origin_reference(image.shape, roi, idx[int(row[17])])
    return (*row[:3], *origin, *row[6:16])


def same(got, want):
    """Exact equality of two arrays; a NaN (the test volumes hold some) equals a NaN."""
    return np.array_equal(got, want, equal_nan=got.dtype.kind == "f")


def same_bits(a, b):
    """Two fp32 tensors of one device hold the same bits (NaN included)."""
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def small_store(device):
    return DeviceVolumeStore([volume(v) for v in range(len(SHAPES))], device)


def misaligned_store(device, vols=(2, 3)):
    """The volumes `vols` at addresses that rule out the 16-byte image load and the 4-byte label load of a full group: the image starts
    4 bytes past a 16-byte boundary, the label 1 byte past a 4-byte boundary."""
    store = DeviceVolumeStore([volume(v) for v in vols], device)
    for i, v in enumerate(vols):
        n = int(np.prod(SHAPES[v]))
        fbuf = torch.empty(n + 8, dtype=torch.float32, device=store.device)
        shift = 1 + (-(fbuf.data_ptr() // 4)) % 4
        image = fbuf[shift:shift + n].view(SHAPES[v])
        bbuf = torch.empty(n + 8, dtype=torch.uint8, device=store.device)
        shift = 1 + (-bbuf.data_ptr()) % 4
        label = bbuf[shift:shift + n].view(SHAPES[v])
        image.copy_(store.images[i])
        label.copy_(store.labels[i])
        assert image.data_ptr() % 16 == 4 and label.data_ptr() % 4 == 1 and image.is_contiguous() and label.is_contiguous()
        store.images[i], store.labels[i] = image, label
    return store


def index_arrays(index, i):
    """(fg, bg) prefix arrays of volume i as int64 numpy (the device words are uint32)."""
    return [t.cpu().numpy().astype(np.int64) & 0xffffffff for t in (index.fg[i], index.bg[i])]


def check_index(store, volumes, threshold=THRESHOLD):
    """ForegroundIndex == numpy's per-tile cumulative counts, totals included; built twice, bit-equal."""
    index = ForegroundIndex(store, threshold)
    again = ForegroundIndex(store, threshold)
    assert _lib.lib().icl_rank_tile() == TILE
    for i, (image, label) in enumerate(volumes):
        want = index_reference(image, label, threshold)
        got = index_arrays(index, i)
        assert index.fg[i].dtype == torch.int32 and len(got[0]) == -(-image.size // TILE) + 1
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (i, image.shape)
        assert index.n_fg[i] == want[0][-1] and index.n_bg[i] == want[1][-1]
        assert torch.equal(index.fg[i], again.fg[i]) and torch.equal(index.bg[i], again.bg[i])
    return index


def special_volumes():
    """An all-zero label | no background at all (image <= threshold wherever the label is 0) | NaN voxels; each on (13, 17, 19)."""
    image, label = volume(2)
    no_fg = (image, np.zeros_like(label))
    no_bg = (np.where(label == 0, -np.abs(np.nan_to_num(image)), image).astype(np.float32), label)
    nans = image.copy()
    nans.reshape(-1)[::5] = np.nan
    return [no_fg, no_bg, (nans, label)]


def raw_select(store, index, samples, roi, batch=None, null=None, origins=None, lo=0):
    """icl_rank_select through ctypes.  samples: (volume, kind, rank[, crop size or None[, extents]]) of one launch; `null`: the argument
    passed as a null pointer.  Returns (rc, origins tensor)."""
    import ctypes
    m = len(samples)
    ptrs = ctypes.c_void_p * m
    vols = [s[0] for s in samples]
    rows = []
    for s in samples:
        shape = tuple(store.images[s[0]].shape)
        size = s[3] if len(s) > 3 and s[3] is not None else [min(r, n) for r, n in zip(roi, shape)]
        rows += [*(s[4] if len(s) > 4 else shape), s[1], s[2], *size]
    args = [ptrs(*[store.images[i].data_ptr() for i in vols]), ptrs(*[store.labels[i].data_ptr() for i in vols]),
            ptrs(*[index.fg[i].data_ptr() for i in vols]), ptrs(*[index.bg[i].data_ptr() for i in vols]), (ctypes.c_int32 * (8 * m))(*rows)]
    if origins is None:
        origins = torch.full((m, 3), -7, dtype=torch.int32, device=store.device)
    out = origins[lo:].data_ptr()
    if null is not None:
        if null < 5:
            args[null] = None
        else:
            out = None
    rc = _lib.lib().icl_rank_select(*args, index.image_threshold, m if batch is None else batch, out, None)
    return rc, origins


def check_select_exhaustive(store, index, v, roi, per_launch=16, slot=None):
    """Every rank of both lists of volume v (entry `slot` of the store, v itself by default), in launches of `per_launch` samples that
    mix the two lists (and ranks from both ends) -> the origin of the reference.  One read-back per volume.  Returns the number of
    samples."""
    image, label = volume(v)
    fg, bg = lists(image, label)
    v = v if slot is None else slot
    assert len(fg) == index.n_fg[v] and len(bg) == index.n_bg[v] and len(fg) and len(bg)
    samples = [(v, KIND_FG, r) for r in range(len(fg))] + [(v, KIND_BG, r) for r in range(len(bg))]
    order = np.arange(len(samples))
    order = np.concatenate([order[0::3], order[1::3][::-1], order[2::3]])      # neighbours in a launch: both lists, far-apart ranks
    samples = [samples[i] for i in order]
    origins = torch.full((len(samples), 3), -7, dtype=torch.int32, device=store.device)
    for lo in range(0, len(samples), per_launch):
        rc, _ = raw_select(store, index, samples[lo:lo + per_launch], roi, origins=origins, lo=lo)
        assert rc == 0, _lib.lib().icl_last_error()
    got = origins.cpu().numpy()
    want = np.array([origin_reference(image.shape, roi, (fg if kind == KIND_FG else bg)[r]) for _, kind, r in samples])
    bad = np.flatnonzero((got != want).any(axis=1))
    assert len(bad) == 0, (v, roi, samples[bad[0]], got[bad[0]], want[bad[0]], len(bad))
    return len(samples)


@functools.lru_cache(maxsize=None)
def end_to_end(roi):
    """B = 5 volume indices x num_samples = 4: 20 samples, two launches.  Ranks at both ends and inside both lists, every k, all flip
    bits, three intensity settings.  Returns (indices, rows, want_image, want_label)."""
    indices = [3, 0, 4, 2, 1]
    rows = []
    for j, v in enumerate(indices):
        image, label = volume(v)
        n_fg, n_bg = (len(x) for x in lists(image, label))
        picks = [(KIND_FG, 0), (KIND_BG, n_bg - 1), (KIND_FG, n_fg - 1), (KIND_BG, n_bg // 2)]
        for q, (kind, rank) in enumerate(picks):
            m = 4 * j + q
            mul, add = aref.INTENSITIES[m % 3]
            rows.append(make_row(SHAPES[v], roi, kind, rank, flip=(m * 3 + 1) % 8, k=m % 4, mul=mul, add=add))
    assert {r[13] for r in rows} == {0, 1, 2, 3} and all(any(r[12] >> a & 1 for r in rows) for a in range(3))
    want = [aref.forward_chain(*volume(v), feed_row(v, row, roi), roi) for v, row in zip([i for i in indices for _ in range(4)], rows)]
    return indices, rows, np.stack([w[0] for w in want]), np.stack([w[1] for w in want])


def check_end_to_end(store, index, roi):
    """OnDeviceAugmentPosNeg.batch with given rows == forward_chain on the reference's crop; out= with both label forms; two runs bit-equal."""
    indices, rows, want_image, want_label = end_to_end(roi)
    feed = OnDeviceAugmentPosNeg(store, index, roi, num_samples=4)
    got = feed.batch(indices, params=rows)
    n = len(rows)
    assert n == 20 and got["image"].shape == (n, 1, *roi) and got["image"].dtype == torch.float32
    assert got["label"].shape == (n, 1, *roi) and got["label"].dtype == torch.int64
    gi, gl = got["image"].cpu().numpy(), got["label"].cpu().numpy()
    for j in range(n):
        assert same(gi[j], want_image[j]), (roi, j, rows[j])
        assert same(gl[j], want_label[j]), (roi, j, rows[j])
    dev = store.device
    image = torch.full((n, 1, *roi), float("nan"), device=dev)
    for label in (torch.full((n, 1, *roi), -1, dtype=torch.int64, device=dev), torch.full((n, *roi), -1, dtype=torch.int64, device=dev)):
        out = feed.batch(indices, params=rows, out=(image, label))
        assert out["image"].data_ptr() == image.data_ptr() and out["label"].data_ptr() == label.data_ptr()
        assert out["label"].shape == (n, 1, *roi)
        assert same_bits(image, got["image"]) and torch.equal(label.view(n, 1, *roi), got["label"])
    assert image.data_ptr() != got["image"].data_ptr()
    return feed


class RecordingRNG:
    """A RandomState that writes down every call: (name, arguments)."""

    def __init__(self, seed):
        self.state = np.random.RandomState(seed)
        self.calls = []

    def rand(self):
        self.calls.append(("rand",))
        return self.state.rand()

    def randint(self, *args):
        self.calls.append(("randint", *args))
        return self.state.randint(*args)

    def uniform(self, lo, hi):
        self.calls.append(("uniform", lo, hi))
        return self.state.uniform(lo, hi)


def documented_draws(seed, shape, roi, n_fg, n_bg, pos=1, neg=1, num_samples=4, flip_prob=0.10, rot_prob=0.10, max_k=3,
                     shift_offset=0.10, shift_prob=0.50, scale_factor=0.0, scale_prob=0.0):
    """The documented sequence, restated on a generator of its own: (rows, calls)."""
    rng = np.random.RandomState(seed)
    calls = []
    ratio = pos / (pos + neg)
    if n_fg == 0:
        ratio = 0
    elif n_bg == 0:
        ratio = 1
    centres = []
    for _ in range(num_samples):
        calls.append(("rand",))
        fg = rng.rand() < ratio
        calls.append(("randint", n_fg if fg else n_bg))
        centres.append((KIND_FG if fg else KIND_BG, int(rng.randint(n_fg if fg else n_bg))))
    size = [min(r, n) for r, n in zip(roi, shape)]
    left = [(r - s) // 2 for r, s in zip(roi, size)]
    rows = []
    for kind, rank in centres:
        flip = 0
        for a in range(3):
            calls.append(("rand",))
            flip |= int(rng.rand() < flip_prob) << a
        calls.append(("rand",))
        k = 0
        if rng.rand() < rot_prob:
            calls.append(("randint", max_k))
            k = int(rng.randint(max_k)) + 1
        mul, add = np.float32(1), np.float32(0)
        if scale_prob > 0:
            calls.append(("rand",))
            if rng.rand() < scale_prob:
                calls.append(("uniform", -scale_factor, scale_factor))
                mul = np.float32(1 + rng.uniform(-scale_factor, scale_factor))
        calls.append(("rand",))
        if rng.rand() < shift_prob:
            calls.append(("uniform", -shift_offset, shift_offset))
            add = np.float32(rng.uniform(-shift_offset, shift_offset))
        rows.append((*shape, 0, 0, 0, *size, *left, flip, k, float(mul), float(add), kind, rank))
    return rows, calls


# ---- the trainer's size: two volumes of amos_feed_ref.BIG_SOURCES' extents with a few blobs of labels (sparse foreground)
BIG_SHAPES = [aref.BIG_SOURCES[0], aref.BIG_SOURCES[3]]          # (130, 101, 70): padded on axis 2 | (60, 200, 111): padded on axis 0


@functools.lru_cache(maxsize=None)
def big_volume(j):
    shape = BIG_SHAPES[j]
    image = hash_uniform_np(int(np.prod(shape)), 90 + j, 1.0).astype(np.float32).reshape(shape)
    label = np.zeros(shape, dtype=np.uint8)
    rng = np.random.RandomState(5 + j)
    grid = np.indices(shape)
    for organ in range(1, 6):                                      # five balls of radius 4..9 voxels
        centre = [int(rng.randint(0, n)) for n in shape]
        radius = int(rng.randint(4, 10))
        label[sum((grid[a] - centre[a]) ** 2 for a in range(3)) <= radius * radius] = organ
    return image, label


@functools.lru_cache(maxsize=None)
def big_batch():
    """2 volumes x 4 samples at 96^3: (indices, rows, want_image, want_label)."""
    rows = []
    for j in range(2):
        image, label = big_volume(j)
        n_fg, n_bg = (len(x) for x in lists(image, label))
        assert 0 < n_fg < image.size // 50                         # sparse
        for q, (kind, rank) in enumerate([(KIND_FG, 0), (KIND_FG, n_fg - 1), (KIND_BG, n_bg // 3), (KIND_FG, n_fg // 2)]):
            m = 4 * j + q
            rows.append(make_row(BIG_SHAPES[j], aref.BIG_ROI, kind, rank, flip=(m * 3 + 1) % 8, k=m % 4, mul=1.0 + 0.0625 * (m % 3), add=0.03125 * (m % 2)))
    want = [aref.forward_chain(*big_volume(j), feed_row(big_volume(j), row, aref.BIG_ROI), aref.BIG_ROI) for j in (0, 1) for row in rows[4 * j:4 * j + 4]]
    return [0, 1], rows, np.stack([w[0] for w in want]), np.stack([w[1] for w in want])
