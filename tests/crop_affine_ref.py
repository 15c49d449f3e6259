"""Shared inputs and checks of the affine stage of the BraTS feed (tests/test_crop_affine_emu.py on the CPU emulator,
tests/test_gpu_crop_affine.py on the GPU; crop_rotflip_affine_kernel in icl_amd/csrc/kernels/datafeed.h, icl_crop_rotflip_affine,
OnDeviceAugment in icl_amd/dataloaders/brats2019.py).  Not a test module.

``crop_affine_chain`` is the yardstick: a literal numpy restatement of DESIGN.md §2 "Affine stage of the BraTS feed" — vectorised, fp64,
the same operations in the same order, every product and sum a numpy operation of its own (numpy never contracts) — on the virtual volume
``Y = flip(rot90(x, k), axis)`` BUILT with ``np.rot90`` / ``np.flip``, where the kernel never materialises it and walks the source with
signed strides.  Every comparison with it is exact (``np.array_equal``).  Parity with MONAI's ``RandAffine`` is unpinned (MONAI is not
installed, and it samples the cropped patch where this gather samples the volume).

Shapes: the sources and the two patches of tests/multimodal_feed_ref.py, and (6, 8, 8), the smallest patch at which the affine path maps
its threads to 8 x 8 tiles.  Odd k on (7, 9, .) exercises the extent swap, (5, 6, 8) fires
the padding rule, (6, 6, 5) takes one voxel per thread and (6, 6, 8) one quad.  References are computed once per case list and shared.
"""
import ctypes
import functools
import itertools

import numpy as np
import torch

import multimodal_feed_ref as mref
from icl_amd import _lib
from icl_amd.dataloaders.amos import affine_matrix
from icl_amd.dataloaders.brats2019 import DeviceVolumeStore, OnDeviceAugment, draw_rotflip_crop
from icl_amd.dataloaders.intensity import IntensityAugment

SOURCES = mref.SOURCES
PATCH_SCALAR = mref.PATCH_SCALAR
PATCH_QUAD = mref.PATCH_QUAD
PATCHES = (PATCH_SCALAR, PATCH_QUAD)
PATCH_TILED = (6, 8, 8)                          # R1 % 8 == 0 and R2 % 8 == 0: an affine sample's waves take 8 x 8 tiles of (rows, depth)
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)
SENTINEL = -7
# the layouts of the identity check: None is a [W,H,D] store (channels = 1 at the entry, compared with icl_crop_rotflip), a number a
# [C,W,H,D] store (compared with icl_crop_rotflip_channels)
IDENTITY_CHANNELS = (None, 1, 2, 3, 4, 16)


def virtual_volume(vol, k, axis):
    """Y = flip(rot90(x, k), axis) of one 3-D array."""
    y = np.rot90(vol, k)
    return np.flip(y, axis=axis) if axis >= 0 else y


def coordinates(row, M, patch):
    """x_a of every output voxel, three float64 arrays of the patch's shape: DESIGN.md's formula, operation by operation."""
    c, p = row[8:11], row[5:8]
    M = np.asarray(M, dtype=np.float64).reshape(3, 3)
    q = np.meshgrid(*[np.arange(r, dtype=np.float64) for r in patch], indexing="ij")
    u = [q[a] - (patch[a] - 1) / 2 for a in range(3)]
    t = [np.float64(int(c[a]) - int(p[a])) + (patch[a] - 1) / 2 for a in range(3)]
    return [t[a] + ((M[a, 0] * u[0] + M[a, 1] * u[1]) + M[a, 2] * u[2]) for a in range(3)]


def crop_affine_chain(image, label, row, M, patch):
    """(image [C, *patch] fp32, label [*patch] int64) of one sample with the affine stage.  ``image``: [C, n0, n1, n2] or [n0, n1, n2];
    ``row``: the 11 integers of draw_rotflip_crop; ``M``: nine values."""
    k, axis = int(row[3]), int(row[4])
    planes = image if image.ndim == 4 else image[None]
    x = coordinates(row, M, patch)
    fl = [np.floor(x[a]) for a in range(3)]
    f = [x[a] - fl[a] for a in range(3)]
    w = [(1.0 - f[a], f[a]) for a in range(3)]
    ylab = virtual_volume(label, k, axis)
    n = ylab.shape
    out = []
    for plane in planes:
        y = virtual_volume(plane, k, axis)
        acc = None
        for bits in itertools.product((0, 1), repeat=3):                 # (0,0,0), (0,0,1), ..., (1,1,1)
            idx = [fl[a] + bits[a] for a in range(3)]
            inside = np.ones(patch, dtype=bool)
            for a in range(3):
                inside &= (idx[a] >= 0) & (idx[a] <= n[a] - 1)
            at = tuple(np.where(inside, idx[a], 0).astype(np.int64) for a in range(3))
            tap = np.where(inside, y[at].astype(np.float64), 0.0)
            term = tap * ((w[0][bits[0]] * w[1][bits[1]]) * w[2][bits[2]])
            acc = term if acc is None else acc + term
        out.append(acc.astype(np.float32))
    rn = [np.rint(x[a]) for a in range(3)]                               # half to even
    inside = np.ones(patch, dtype=bool)
    for a in range(3):
        inside &= (rn[a] >= 0) & (rn[a] <= n[a] - 1)
    at = tuple(np.where(inside, rn[a], 0).astype(np.int64) for a in range(3))
    return np.stack(out), np.where(inside, ylab[at], 0).astype(np.int64)


# ---- data ------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def random_volumes(channels):
    """[(image fp32 [channels, *shape] (or [*shape] with None), label uint8)] of the three sources: uniform values in (-1, 3) plus 10 c in
    channel c (no voxel is 0, a wrong channel is off by 10), labels 0..5."""
    out = []
    for tag, shape in enumerate(SOURCES):
        rng = np.random.RandomState(70 + tag)
        planes = [(rng.uniform(-1.0, 3.0, size=shape) + 10.0 * c).astype(np.float32) for c in range(channels or 1)]
        image = np.ascontiguousarray(np.stack(planes) if channels is not None else planes[0])
        out.append((image, rng.randint(0, 6, size=shape).astype(np.uint8)))
    return out


def to_tensors(volumes, device):
    return [(torch.as_tensor(i).to(device), torch.as_tensor(l).to(device)) for i, l in volumes]


def random_origin_row(rng, shape, k, axis, patch):
    dims, pads = mref.pads_for(shape, k, patch)
    span = [dims[a] + 2 * pads[a] - patch[a] for a in range(3)]
    return (*shape, k, axis, *pads, *[int(rng.randint(0, span[a])) for a in range(3)])


@functools.lru_cache(maxsize=None)
def random_cases(patch):
    """(source index, row, M): four per source, the twelve (k, axis) pairs once each; rotations up to +-0.6 rad, zooms in 0.7 .. 1.4,
    anisotropic for two of the four and isotropic for the others; seeded."""
    rng = np.random.RandomState(30 + patch[2])
    cases = []
    for si, shape in enumerate(SOURCES):
        for q in range(4):
            k, axis = mref.ROTFLIPS[(4 * si + q) % 12]
            zoom = rng.uniform(0.7, 1.4, 3) if q % 2 == 0 else rng.uniform(0.7, 1.4)
            M = affine_matrix(rng.uniform(-0.6, 0.6, 3), zoom)
            cases.append((si, random_origin_row(rng, shape, k, axis, patch), tuple(M.reshape(-1))))
    assert len({(c[1][3], c[1][4]) for c in cases}) == 12
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def dyadic_cases(patch):
    """Zoom 1/2 (M = diag(2)) and zoom 2 (M = diag(1/2)) on every source, k and flip varying.  With u a half-integer (extent 6 or 8)
    diag(2) lands on exact halves, with u an integer (extent 5) diag(1/2) does: f = 0.5 for the image, half-to-even for the label."""
    rng = np.random.RandomState(40 + patch[2])
    cases = []
    for si, shape in enumerate(SOURCES):
        for j, z in enumerate((2.0, 0.5)):
            k, axis = mref.ROTFLIPS[(5 * si + 7 * j + 1) % 12]
            cases.append((si, random_origin_row(rng, shape, k, axis, patch), tuple(np.diag([z] * 3).reshape(-1))))
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def reference(cases, patch, channels):
    """The restatement of a tuple of cases on random_volumes(channels), once: (image [N, C, *patch], label [N, *patch])."""
    vols = random_volumes(channels)
    want = [crop_affine_chain(*vols[si], row, M, patch) for si, row, M in cases]
    return np.stack([w[0] for w in want]), np.stack([w[1] for w in want])


# ---- the raw entry point ---------------------------------------------------------------------------------------------------------------

_KEEP = []


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream) if dev.type == "cuda" else None


def sentinel_outputs(m, channels, patch, device, misaligned=False):
    """(image [m, channels, *patch], label [m, *patch]) filled with SENTINEL.  ``misaligned``: the image starts 4 bytes past a 16-byte
    boundary, which rules out the 16-byte stores (the launcher must take the one-voxel kernel)."""
    per = max(int(np.prod(patch)), 1)
    ibuf = torch.full((m * channels * per + 8,), float(SENTINEL), dtype=torch.float32, device=device)
    shift = (-(ibuf.data_ptr() // 4)) % 4 + (1 if misaligned else 0)
    image = ibuf[shift:shift + m * channels * per]
    label = torch.full((m * per,), SENTINEL, dtype=torch.int64, device=device)
    assert image.data_ptr() % 16 == (4 if misaligned else 0)
    if int(np.prod(patch)) > 0:
        image, label = image.view(m, channels, *patch), label.view(m, *patch)
    return image, label


def raw_affine(lib, tensors, items, mats, channels, patch, flags=None, misaligned=False, batch=None, null=None):
    """One icl_crop_rotflip_affine launch through ctypes on sentinel-filled outputs.  ``tensors``: [(image, label)] on the device;
    ``items``: [(source index, row)]; ``mats``: nine values per sample; ``flags``: default 1 for every sample; ``null``: the pointer
    argument to pass as NULL (0 images, 1 labels, 2 params, 3 affine_params, 4 image_out, 5 label_out).  Returns (rc, image, label)."""
    m = len(items)
    dev = tensors[0][0].device
    ptrs = ctypes.c_void_p * m
    flags = [1.0] * m if flags is None else flags
    image, label = sentinel_outputs(m, max(channels, 1), patch, dev, misaligned)
    args = [ptrs(*[tensors[si][0].data_ptr() for si, _ in items]), ptrs(*[tensors[si][1].data_ptr() for si, _ in items]),
            (ctypes.c_int32 * (11 * m))(*[int(v) for _, row in items for v in row]),
            (ctypes.c_double * (10 * m))(*[float(v) for flag, M in zip(flags, mats) for v in (flag, *M)]),
            image.data_ptr(), label.data_ptr()]
    if null is not None:
        args[null] = None
    _KEEP.append((args, image, label))
    rc = lib.icl_crop_rotflip_affine(*args[:4], m if batch is None else batch, channels, *args[4:], *patch, _stream(dev))
    return rc, image, label


def raw_plain(lib, tensors, items, channels, patch, misaligned=False):
    """The same samples through the entry without the stage: icl_crop_rotflip for a [W,H,D] store (``channels`` None), else
    icl_crop_rotflip_channels."""
    entry = "icl_crop_rotflip" if channels is None else "icl_crop_rotflip_channels"
    rc, image, label = mref.raw_channels(lib, tensors, items, channels or 1, patch, misaligned, entry=entry)
    assert rc == 0, lib.icl_last_error()
    return image, label


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def run_cases(lib, tensors, cases, channels, patch, misaligned=False, per_launch=16):
    images, labels = [], []
    for lo in range(0, len(cases), per_launch):
        part = cases[lo:lo + per_launch]
        rc, image, label = raw_affine(lib, tensors, [(c[0], c[1]) for c in part], [c[2] for c in part], channels, patch, misaligned=misaligned)
        assert rc == 0, lib.icl_last_error()
        images.append(image.cpu().numpy())
        labels.append(label.cpu().numpy())
    _KEEP.clear()
    return np.concatenate(images), np.concatenate(labels)


def check_cases(got, cases, want):
    for j, case in enumerate(cases):
        for c in range(want[0].shape[1]):
            assert np.array_equal(got[0][j, c], want[0][j, c]), ("image", j, c, case)
        assert np.array_equal(got[1][j], want[1][j]), ("label", j, case)


# ---- 1. identity -----------------------------------------------------------------------------------------------------------------------

def check_identity(lib, device, channels, patch, misaligned=False):
    """multimodal_feed_ref's sweep (3 sources x 12 (k, axis) pairs x the depth origins, 16 mixed samples a launch): every sample with
    flag 1 and M = I equals the plain entry bit for bit, and the forward chain.  Returns the number of samples."""
    volumes = mref.make_store_arrays(channels)
    tensors = to_tensors(volumes, device)
    items = mref.sweep_rows(patch)
    assert {(row[3], row[4]) for _, row in items} == set(mref.ROTFLIPS)
    want_image, want_label = mref.expected(volumes, items, patch)
    for lo in range(0, len(items), 16):
        part = items[lo:lo + 16]
        rc, image, label = raw_affine(lib, tensors, part, [IDENTITY] * len(part), channels or 1, patch, misaligned=misaligned)
        assert rc == 0, lib.icl_last_error()
        plain_image, plain_label = raw_plain(lib, tensors, part, channels, patch, misaligned)
        assert same_bits(image, plain_image) and torch.equal(label, plain_label), (lo, channels, patch)
        assert np.array_equal(image.cpu().numpy(), want_image[lo:lo + 16]) and np.array_equal(label.cpu().numpy(), want_label[lo:lo + 16])
    _KEEP.clear()
    mref._KEEP.clear()
    return len(items)


# ---- 2. flag 0 in a mixed launch -------------------------------------------------------------------------------------------------------

def check_mixed_flags(lib, device, channels, patch):
    """16 samples, flags 0, 1, 0, 1, ...: the flag-0 samples (whose M is a legal matrix that must not be read) equal the plain kernel's,
    the others the restatement."""
    cases = (random_cases(patch) + dyadic_cases(patch))[:16]
    assert len(cases) == 16
    tensors = to_tensors(random_volumes(channels), device)
    items = [(c[0], c[1]) for c in cases]
    flags = [float(j % 2) for j in range(16)]
    rc, image, label = raw_affine(lib, tensors, items, [c[2] for c in cases], channels or 1, patch, flags=flags)
    assert rc == 0, lib.icl_last_error()
    plain_image, plain_label = raw_plain(lib, tensors, items, channels, patch)
    want = reference(cases, patch, channels)
    gi, gl = image.cpu().numpy(), label.cpu().numpy()
    for j in range(16):
        if flags[j] == 0.0:
            assert same_bits(image[j], plain_image[j]) and torch.equal(label[j], plain_label[j]), j
        else:
            assert np.array_equal(gi[j], want[0][j]) and np.array_equal(gl[j], want[1][j]), j
            assert not same_bits(image[j], plain_image[j]), j
    _KEEP.clear()
    mref._KEEP.clear()


# ---- 3. against the single-channel kernel on the materialised Y -----------------------------------------------------------------------

def check_against_volume_feed_affine(lib, device, patch, channels=3, misaligned_amos=False):
    """Y = flip(rot90(x, k), axis) is materialised on the host for each channel and goes through icl_volume_feed_affine with origin
    max(c - p, 0), left pad max(p - c, 0), the matching size, no flips, k = 0, mul = 1, add = 0 and the same M (so t_a is the same
    number): this kernel on x equals it channel by channel; the label is compared once.  ``misaligned_amos``: the outputs of the
    single-channel entry are 4 bytes off, so the two sides run the shared sampler from different instances (V = 1 there).  Returns the
    number of cases."""
    cases = random_cases(patch)
    vols = random_volumes(channels)
    got = run_cases(lib, to_tensors(vols, device), list(cases), channels, patch)
    one = ctypes.c_void_p * 1
    for j, (si, row, M) in enumerate(cases):
        k, axis = row[3], row[4]
        ylab = np.ascontiguousarray(virtual_volume(vols[si][1], k, axis))
        n = ylab.shape
        origin = [max(row[8 + a] - row[5 + a], 0) for a in range(3)]
        left = [max(row[5 + a] - row[8 + a], 0) for a in range(3)]
        size = [min(patch[a] - left[a], n[a] - origin[a]) for a in range(3)]
        assert min(size) >= 1 and all(origin[a] - left[a] == row[8 + a] - row[5 + a] for a in range(3))
        ints = (ctypes.c_int32 * 14)(*n, *origin, *size, *left, 0, 0)
        floats = (ctypes.c_float * 2)(1.0, 0.0)
        affine = (ctypes.c_double * 10)(1.0, *M)
        tlab = torch.as_tensor(ylab).to(device)
        for c in range(channels):
            timg = torch.as_tensor(np.ascontiguousarray(virtual_volume(vols[si][0][c], k, axis))).to(device)
            image, label = sentinel_outputs(1, 1, patch, device, misaligned_amos)
            rc = lib.icl_volume_feed_affine(one(timg.data_ptr()), one(tlab.data_ptr()), ints, floats, affine, 1, image.data_ptr(),
                                            label.data_ptr(), *patch, _stream(device))
            assert rc == 0, lib.icl_last_error()
            assert np.array_equal(got[0][j, c], image[0, 0].cpu().numpy()), (j, c, row, M)
            if c == 0:
                assert np.array_equal(got[1][j], label[0].cpu().numpy()), (j, row, M)
    return len(cases)


# ---- 4. the numpy reference ------------------------------------------------------------------------------------------------------------

def check_reference(lib, device, patch, channels=3):
    """The random cases, aligned outputs (the quad kernel where R2 % 4 == 0) and outputs 4 bytes off (the one-voxel kernel), and the
    dyadic zooms, which must hit f = 0.5 and a rint tie."""
    tensors = to_tensors(random_volumes(channels), device)
    cases = random_cases(patch)
    want = reference(cases, patch, channels)
    for misaligned in (False, True):
        check_cases(run_cases(lib, tensors, list(cases), channels, patch, misaligned=misaligned), cases, want)
    dyadic = dyadic_cases(patch)
    halves = 0
    for _, row, M in dyadic:
        for x in coordinates(row, M, patch):
            halves += int(((x - np.floor(x)) == 0.5).sum())
    assert halves > 0
    check_cases(run_cases(lib, tensors, list(dyadic), channels, patch), dyadic, reference(dyadic, patch, channels))
    return len(cases) + len(dyadic)


def check_nonfinite(lib, device, patch, channels=2):
    """Voxel (0, 0, 0) of every channel, which stands in for a tap outside the volume inside the kernel, holds a NaN; the last voxel
    holds +inf and one interior voxel -inf.  A tap outside counts as 0 whatever the stand-in holds, a tap inside carries its value even
    where its weight is 0 (0 * inf is a NaN in the definition too): equal to the restatement, a NaN equal to a NaN."""
    vols = []
    for image, label in random_volumes(channels):
        image = image.copy()
        image[:, 0, 0, 0] = np.nan
        image[:, -1, -1, -1] = np.inf
        image[:, image.shape[1] // 2, image.shape[2] // 2, image.shape[3] // 2] = -np.inf
        vols.append((image, label))
    cases = random_cases(patch) + dyadic_cases(patch)
    got = run_cases(lib, to_tensors(vols, device), list(cases), channels, patch)
    nans = zeros = 0
    for j, (si, row, M) in enumerate(cases):
        with np.errstate(invalid="ignore"):                              # 0 * inf and inf - inf are part of the case
            want_image, want_label = crop_affine_chain(*vols[si], row, M, patch)
        assert np.array_equal(got[0][j], want_image, equal_nan=True), (j, row, M)
        assert np.array_equal(got[1][j], want_label), (j, row, M)
        nans += int(np.isnan(want_image).sum())
        zeros += int((want_image == 0).sum())
    assert nans > 0 and zeros > 0


def check_single_channel_store(lib, device, patch):
    """A [W,H,D] store passes channels = 1: the result is channel 0 of the [C,W,H,D] run, and the restatement."""
    cases = random_cases(patch)
    got = run_cases(lib, to_tensors(random_volumes(None), device), list(cases), 1, patch)
    check_cases(got, cases, reference(cases, patch, None))


# ---- 5. scipy --------------------------------------------------------------------------------------------------------------------------

def check_scipy(lib, device, patch, channels=2):
    """scipy.ndimage.affine_transform(order=1, mode="grid-constant", cval=0) of Y in float64 with matrix M and offset t - M ctr, one case
    per patch, image only.  scipy keeps the sum in double, the kernel rounds it once to fp32: the band is 2^-23 max|image|."""
    from scipy import ndimage
    case = random_cases(patch)[5]
    si, row, M = case
    vols = random_volumes(channels)
    got = run_cases(lib, to_tensors(vols, device), [case], channels, patch)[0][0]
    M = np.asarray(M).reshape(3, 3)
    ctr = (np.asarray(patch, dtype=np.float64) - 1) / 2
    t = np.asarray(row[8:11], dtype=np.float64) - np.asarray(row[5:8], dtype=np.float64) + ctr
    for c in range(channels):
        y = virtual_volume(vols[si][0][c], row[3], row[4]).astype(np.float64)
        want = ndimage.affine_transform(y, M, offset=t - M @ ctr, output_shape=patch, order=1, mode="grid-constant", cval=0.0)
        worst = float(np.abs(got[c].astype(np.float64) - want).max())
        bound = 2.0 ** -23 * float(np.abs(vols[si][0][c]).max())
        print(f"patch {patch} channel {c}: image |diff| {worst:.3e} (bound {bound:.3e})")
        assert worst <= bound, (patch, c, worst, bound)
        assert np.abs(want).max() > 1.0                                  # the case samples the volume, not only the zeros around it


# ---- 6. loader -------------------------------------------------------------------------------------------------------------------------

class Spy:
    """Stands in for the library and records the names of the crop entries that are looked up for a call."""

    def __init__(self, lib, calls):
        self._lib, self._calls = lib, calls

    def __getattr__(self, name):
        if name.startswith("icl_crop_rotflip"):
            self._calls.append(name)
        return getattr(self._lib, name)


AFFINE_KW = dict(affine_prob=1.0, rotate_range=(0.6, 0.5, 0.4), zoom_range=(0.7, 1.4), zoom_isotropic=False)


def check_loader(device, monkeypatch, channels):
    """OnDeviceAugment over a [W,H,D] (``channels`` None) or [C,W,H,D] store of the random volumes."""
    import pytest
    vols = random_volumes(channels)
    store = DeviceVolumeStore(vols, device)
    patch = PATCH_QUAD
    old_entry = "icl_crop_rotflip" if channels is None else "icl_crop_rotflip_channels"
    calls = []
    lib = _lib.lib()
    monkeypatch.setattr(_lib, "lib", lambda: Spy(lib, calls))
    idx = [2, 0, 1, 1, 0]

    # affine_prob = 0: the draws, the launch and the bits of a feed without the keywords
    np.random.seed(41)
    rows = [draw_rotflip_crop(vols[i][0].shape[-3:], patch) for i in idx]
    after = np.random.randint(1 << 30)
    for feed in (OnDeviceAugment(store, patch), OnDeviceAugment(store, patch, affine_prob=0.0, rotate_range=0.5, zoom_range=(0.7, 1.4))):
        del calls[:]
        np.random.seed(41)
        got = feed.batch(idx)
        assert np.random.randint(1 << 30) == after                      # nothing else was drawn
        assert calls == [old_entry]
        want_image, want_label = mref.expected(vols, [(i, rows[j]) for j, i in enumerate(idx)], patch)
        assert np.array_equal(got["image"].cpu().numpy(), want_image) and np.array_equal(got["label"].cpu().numpy(), want_label)

    # affine_prob = 1: the draw of a sample follows its draw_rotflip_crop directly; a batch drawn inside batch() equals the one given its rows
    feed = OnDeviceAugment(store, patch, **AFFINE_KW)
    np.random.seed(43)
    drawn = feed.draw(idx)
    np.random.seed(43)
    by_hand = []
    for i in idx:
        row = draw_rotflip_crop(vols[i][0].shape[-3:], patch)
        assert np.random.rand() < 1.0
        theta = [np.random.uniform(-r, r) for r in AFFINE_KW["rotate_range"]]
        zoom = [np.random.uniform(0.7, 1.4) for _ in range(3)]
        by_hand.append(row + [float(v) for v in affine_matrix(theta, zoom).reshape(-1)])
    assert drawn == by_hand and all(len(r) == 20 for r in drawn)
    del calls[:]
    given = feed.batch(idx, params=drawn)
    np.random.seed(43)
    inside = feed.batch(idx)
    assert calls == ["icl_crop_rotflip_affine"] * 2
    assert same_bits(given["image"], inside["image"]) and torch.equal(given["label"], inside["label"])
    assert given["image"].shape == (5, channels or 1, *patch) and given["label"].shape == (5, *patch) and given["label"].dtype == torch.int64
    for j, i in enumerate(idx):
        want = crop_affine_chain(*vols[i], drawn[j][:11], drawn[j][11:], patch)
        assert np.array_equal(given["image"][j].cpu().numpy(), want[0]) and np.array_equal(given["label"][j].cpu().numpy(), want[1]), j

    # 17 samples: two launches; a second launch in which no row has a matrix is the old entry
    idx17 = [j % 3 for j in range(17)]
    np.random.seed(44)
    rows17 = feed.draw(idx17)
    del calls[:]
    all17 = feed.batch(idx17, params=rows17)
    assert calls == ["icl_crop_rotflip_affine"] * 2
    del calls[:]
    mixed = feed.batch(idx17, params=rows17[:16] + [rows17[16][:11]])
    assert calls == ["icl_crop_rotflip_affine", old_entry]
    assert same_bits(all17["image"][:16], mixed["image"][:16]) and torch.equal(all17["label"][:16], mixed["label"][:16])
    want = mref.expected(vols, [(idx17[16], rows17[16][:11])], patch)
    assert np.array_equal(mixed["image"][16].cpu().numpy(), want[0][0]) and np.array_equal(mixed["label"][16].cpu().numpy(), want[1][0])
    want = crop_affine_chain(*vols[idx17[16]], rows17[16][:11], rows17[16][11:], patch)
    assert np.array_equal(all17["image"][16].cpu().numpy(), want[0]) and np.array_equal(all17["label"][16].cpu().numpy(), want[1])

    # bad rows: ValueError before anything travels
    good = drawn[0]
    for bad, match in ((good[:13] + [float("nan")] + good[14:], "M\\[0\\]\\[2\\] = nan must be finite"),
                       (good[:15] + [16.5] + good[16:], "M\\[1\\]\\[1\\] = 16.5 must be finite and at most 16"),
                       (good[:15], "one parameter row of 11 values per index \\(20 with an affine matrix\\); row 1 has 15")):
        del calls[:]
        with pytest.raises(ValueError, match=match):
            feed.batch([idx[0], idx[0]], params=[good, bad])
        assert calls == []
    other = next(r for j, r in enumerate(drawn) if idx[j] != idx[0])
    with pytest.raises(ValueError, match="names the extents"):
        feed.batch([idx[0]], params=[other])                             # the row of another volume
    assert calls == []
    for kw in (dict(affine_prob=1.5), dict(rotate_range=(0.1, -0.1, 0.0)), dict(zoom_range=(1.2, 0.8))):
        with pytest.raises(ValueError):
            OnDeviceAugment(store, patch, **kw)

    # the intensity stage behind the affine: its rows are drawn after all geometric rows, per channel on [B, C, ...]
    kw = dict(contrast_prob=1.0, noise_prob=1.0)
    stage = IntensityAugment(patch, rng=np.random.RandomState(8), **kw)
    assert stage.per_channel
    both = OnDeviceAugment(store, patch, intensity=stage, **AFFINE_KW)
    np.random.seed(43)
    got = both.batch(idx)
    replay = IntensityAugment(patch, rng=np.random.RandomState(8), **kw)
    irows = replay.draw(5, channels=channels or 1)
    assert len(irows) == 5 * (channels or 1)
    want = replay.apply(given["image"].clone(), irows)
    assert same_bits(got["image"], want) and torch.equal(got["label"], given["label"])
    assert not same_bits(got["image"], given["image"])


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------------

def check_refusals(lib, device):
    """Every refusal of icl_crop_rotflip_channels and the affine refusals of icl_volume_feed_affine: -1, a message that names the sample
    and the entry, outputs untouched."""
    import pytest
    patch = PATCH_QUAD
    tensors = to_tensors(random_volumes(2), device)
    cases = random_cases(patch)[:3]
    items, mats = [(c[0], c[1]) for c in cases], [c[2] for c in cases]
    rc, image, label = raw_affine(lib, tensors, items, mats, 2, patch)
    assert rc == 0 and not (image == SENTINEL).any() and not (label == SENTINEL).any()

    def refused(match, items_=items, mats_=mats, channels=2, patch_=patch, **kw):
        rc, image, label = raw_affine(lib, tensors, items_, mats_, channels, patch_, **kw)
        assert rc == -1
        with pytest.raises(RuntimeError, match=match):
            _lib.check(rc, "crop_rotflip_affine")
        assert (image == SENTINEL).all() and (label == SENTINEL).all()

    def with_entry(e, value):
        return IDENTITY[:e] + (value,) + IDENTITY[e + 1:]

    for null in (0, 1, 2, 4, 5):
        refused("crop_rotflip_affine: null pointer", null=null)
    refused("crop_rotflip_affine: affine_params is a null pointer", null=3)
    refused("channels 0 out of range", channels=0)
    refused("channels 17 out of range", channels=17)
    refused("batch 0 out of range", batch=0)
    refused("batch 17 out of range", items_=(items * 6)[:16], mats_=(mats * 6)[:16], batch=17)
    si, row = items[0]
    refused("bad sample 1", items_=[items[0], (si, row[:3] + (4,) + row[4:])], mats_=mats[:2])                # k = 4
    refused("bad sample 0", items_=[(si, row[:5] + (-1,) + row[6:])], mats_=mats[:1])                         # negative padding
    refused("output extents", patch_=(6, 6, 0))
    refused("crop_rotflip_affine: sample 0: affine matrix entry M\\[0\\]\\[1\\] = nan is not finite", mats_=[with_entry(1, float("nan"))] + mats[1:])
    refused("sample 1: affine matrix entry M\\[2\\]\\[2\\] = inf is not finite", mats_=[mats[0], with_entry(8, float("inf")), mats[2]])
    refused("affine matrix entry M\\[1\\]\\[0\\] = -inf is not finite", mats_=[with_entry(3, float("-inf"))] + mats[1:])
    refused("sample 2: affine matrix entry M\\[1\\]\\[2\\] = 16.5 outside \\[-16, 16\\]", mats_=mats[:2] + [with_entry(5, 16.5)])
    refused("affine matrix entry M\\[0\\]\\[0\\] = -16.5 outside", mats_=[with_entry(0, -16.5)] + mats[1:])
    refused("sample 0: affine matrix entry M\\[0\\]\\[1\\] = nan", mats_=[with_entry(1, float("nan"))] + mats[1:], flags=[0.0, 1.0, 1.0])
    refused("sample 1: affine flag 2 \\(must be 0 or 1\\)", flags=[1.0, 2.0, 1.0])
    refused("affine flag 0.5", flags=[0.5, 1.0, 1.0])
    refused("affine flag nan", flags=[float("nan"), 1.0, 1.0])
    rc, image, label = raw_affine(lib, tensors, items[:1], [with_entry(4, 16.0)], 2, patch)                   # the bound itself is legal
    assert rc == 0 and not (image == SENTINEL).any()
    # a null volume pointer inside the pointer arrays
    one = ctypes.c_void_p * 1
    image, label = sentinel_outputs(1, 2, patch, device)
    rc = lib.icl_crop_rotflip_affine(one(None), one(tensors[si][1].data_ptr()), (ctypes.c_int32 * 11)(*row), (ctypes.c_double * 10)(1.0, *IDENTITY),
                                     1, 2, image.data_ptr(), label.data_ptr(), *patch, _stream(device))
    assert rc == -1 and b"sample 0: null volume pointer" in lib.icl_last_error() and (image == SENTINEL).all() and (label == SENTINEL).all()
    _KEEP.clear()
