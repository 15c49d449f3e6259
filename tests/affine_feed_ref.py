"""Shared inputs and checks of the affine stage of the 3-D feed (tests/test_affine_feed_emu.py on the CPU emulator,
tests/test_gpu_affine_feed.py on the GPU; volume_feed_affine_kernel in icl_amd/csrc/kernels/datafeed.h, icl_volume_feed_affine /
icl_volume_feed_affine_origins, icl_amd/dataloaders/amos.py).  Not a test module.

``affine_chain`` is the yardstick: a literal numpy restatement of DESIGN.md §2 "Affine stage of the 3-D feed" — vectorised, fp64, the
same operations in the same order, every product and sum a numpy operation of its own (numpy never contracts) — evaluated on the PATCH
grid and then flipped and turned FORWARDS with ``np.flip`` / ``np.rot90``, the opposite formulation from the kernel, which maps every
output voxel backwards.  Every comparison with it is exact (``np.array_equal``).  Parity with MONAI's ``RandAffine`` is unpinned (MONAI
is not installed, and it samples the cropped patch where this gather samples the volume).

References are computed once per case list and shared.
"""
import ctypes
import functools
import itertools

import numpy as np
import torch

import amos_feed_ref as aref
from icl_amd import _lib
from icl_amd.dataloaders.amos import OnDeviceAugmentAMOS, affine_matrix
from icl_amd.dataloaders.brats2019 import DeviceVolumeStore

ROI_SCALAR = aref.ROI_SCALAR          # (6, 6, 5): one thread per voxel
ROI_QUAD = aref.ROI_QUAD              # (6, 6, 8): one thread per four depth voxels on the integer path
ROI_TILED = (8, 8, 8)                 # R1 % 8 == 0 and R2 % 8 == 0: an affine sample's waves take 8 x 8 tiles of (rows, depth); two workgroups
ROIS = (ROI_SCALAR, ROI_QUAD, ROI_TILED)
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)
CUBES = [(8, 8, 8), (5, 5, 5)]        # source == roi: the quad path with an even centre (3.5), the scalar path with an odd one (2)
RANDOM_SOURCES = [(7, 5, 9), (12, 11, 4), (9, 9, 8), (13, 12, 11)]
RANDOM_ROIS = [ROI_TILED, ROI_SCALAR]


def coordinates(row, M, roi):
    """x_a of every voxel of the PATCH grid (before the flips and the quarter turn), three float64 arrays: the formula, operation by
    operation."""
    c, left = row[3:6], row[9:12]
    M = np.asarray(M, dtype=np.float64).reshape(3, 3)
    p = np.meshgrid(*[np.arange(r, dtype=np.float64) for r in roi], indexing="ij")
    u = [p[a] - (roi[a] - 1) / 2 for a in range(3)]
    t = [np.float64(int(c[a]) - int(left[a])) + (roi[a] - 1) / 2 for a in range(3)]
    return [t[a] + ((M[a, 0] * u[0] + M[a, 1] * u[1]) + M[a, 2] * u[2]) for a in range(3)]


def forwards(y, row):
    """A patch-grid array through the flips and the quarter turn of ``row``, forwards."""
    for a in range(3):
        if int(row[12]) >> a & 1:
            y = np.flip(y, a)
    return np.rot90(y, int(row[13]), axes=(0, 1))


def affine_chain(image, label, row, M, roi):
    """(image [1, *roi] fp32, label [1, *roi] int64) of one sample with the affine stage.  ``row``: the 16 feed values; ``M``: 3x3."""
    n = image.shape
    mul, add = np.float32(row[14]), np.float32(row[15])
    x = coordinates(row, M, roi)
    fl = [np.floor(x[a]) for a in range(3)]
    f = [x[a] - fl[a] for a in range(3)]
    w = [(1.0 - f[a], f[a]) for a in range(3)]
    acc = None
    for bits in itertools.product((0, 1), repeat=3):                     # (0,0,0), (0,0,1), ..., (1,1,1)
        idx = [fl[a] + bits[a] for a in range(3)]
        inside = np.ones(roi, dtype=bool)
        for a in range(3):
            inside &= (idx[a] >= 0) & (idx[a] <= n[a] - 1)
        at = tuple(np.where(inside, idx[a], 0).astype(np.int64) for a in range(3))
        tap = np.where(inside, image[at].astype(np.float64), 0.0)
        term = tap * ((w[0][bits[0]] * w[1][bits[1]]) * w[2][bits[2]])
        acc = term if acc is None else acc + term
    img = acc.astype(np.float32)
    rn = [np.rint(x[a]) for a in range(3)]                               # half to even
    inside = np.ones(roi, dtype=bool)
    for a in range(3):
        inside &= (rn[a] >= 0) & (rn[a] <= n[a] - 1)
    at = tuple(np.where(inside, rn[a], 0).astype(np.int64) for a in range(3))
    lab = np.where(inside, label[at], 0).astype(np.int64)
    y = (forwards(img, row) * mul).astype(np.float32)        # rounded ...
    y = (y + add).astype(np.float32)                         # ... and rounded again
    return np.ascontiguousarray(y)[None], np.ascontiguousarray(forwards(lab, row))[None]


def same(got, want):
    """Exact equality of two arrays; a NaN (the pos/neg volumes hold some) equals a NaN."""
    return np.array_equal(got, want, equal_nan=got.dtype.kind == "f")


# ---- the raw entry points -------------------------------------------------------------------------------------------------------------

SENTINEL = -7
_KEEP = []


def sentinel_outputs(m, roi, device, misaligned=False):
    """(image [m,1,*roi], label [m,*roi]) filled with SENTINEL.  ``misaligned``: the image starts 4 bytes and the label 8 bytes past a
    16-byte boundary, which rules out the 16-byte stores (the launcher must take the one-voxel kernel)."""
    per = roi[0] * roi[1] * roi[2]
    ibuf = torch.full((m * per + 8,), float(SENTINEL), dtype=torch.float32, device=device)
    lbuf = torch.full((m * per + 4,), SENTINEL, dtype=torch.int64, device=device)
    ishift = (-(ibuf.data_ptr() // 4)) % 4 + (1 if misaligned else 0)
    lshift = (-(lbuf.data_ptr() // 8)) % 2 + (1 if misaligned else 0)
    image = ibuf[ishift:ishift + m * per].view(m, 1, *roi)
    label = lbuf[lshift:lshift + m * per].view(m, *roi)
    assert image.data_ptr() % 16 == (4 if misaligned else 0) and label.data_ptr() % 16 == (8 if misaligned else 0)
    return image, label


def raw_affine(store, roi, indices, rows, mats, flags=None, misaligned=False, null_affine=False, origins=None):
    """icl_volume_feed_affine (``origins`` None) or icl_volume_feed_affine_origins (``origins``: an int32 [m][3] tensor on the store's
    device) through ctypes with sentinel-filled outputs.  ``mats``: nine values per sample; ``flags``: default 1 for every sample.
    Returns (rc, image [m,1,*roi], label [m,*roi])."""
    m = len(rows)
    ptrs = ctypes.c_void_p * m
    flags = [1.0] * m if flags is None else flags
    affine = (ctypes.c_double * (10 * m))(*[float(v) for flag, M in zip(flags, mats) for v in (flag, *np.asarray(M, dtype=np.float64).reshape(-1))])
    image, label = sentinel_outputs(m, roi, store.device, misaligned)
    args = [ptrs(*[store.images[i].data_ptr() for i in indices]), ptrs(*[store.labels[i].data_ptr() for i in indices]),
            (ctypes.c_int32 * (14 * m))(*[int(v) for r in rows for v in r[:14]]), (ctypes.c_float * (2 * m))(*[float(v) for r in rows for v in r[14:16]]),
            None if null_affine else affine, m]
    stream = ctypes.c_void_p(torch.cuda.current_stream(store.device).cuda_stream) if store.device.type == "cuda" else None
    _KEEP.append((args, image, label, origins))
    L = _lib.lib()
    if origins is None:
        rc = L.icl_volume_feed_affine(*args, image.data_ptr(), label.data_ptr(), *roi, stream)
    else:
        rc = L.icl_volume_feed_affine_origins(*args, origins.data_ptr(), image.data_ptr(), label.data_ptr(), *roi, stream)
    return rc, image, label


def run_cases(store, roi, cases, misaligned=False, per_launch=16):
    """``cases``: (volume index, 16-value row, M) each, of one roi -> (image [N,1,*roi], label [N,1,*roi]) numpy, through the raw entry
    point in launches of ``per_launch``."""
    images, labels = [], []
    for lo in range(0, len(cases), per_launch):
        part = cases[lo:lo + per_launch]
        rc, image, label = raw_affine(store, roi, [c[0] for c in part], [c[1] for c in part], [c[2] for c in part], misaligned=misaligned)
        assert rc == 0, _lib.lib().icl_last_error()
        images.append(image.cpu().numpy())
        labels.append(label.cpu().numpy()[:, None])
    return np.concatenate(images), np.concatenate(labels)


def check_cases(got, cases, want):
    for j, case in enumerate(cases):
        assert same(got[0][j], want[0][j]), ("image", j, case[1], case[2])
        assert same(got[1][j], want[1][j]), ("label", j, case[1], case[2])


# ---- 1. identity ----------------------------------------------------------------------------------------------------------------------

def check_identity(store, roi):
    """amos_feed_ref's sweep (3 sources x 8 flip masks x 4 rotations x 3 intensity pairs; padding on one, two and three axes): each row
    with M = I appended, through icl_volume_feed_affine, equals icl_volume_feed on the plain row bit for bit (and the forward chain)."""
    indices, rows, want_image, want_label = aref.sweep(roi)
    feed = OnDeviceAugmentAMOS(store, roi)
    for lo in range(0, len(indices), 16):
        idx, par = indices[lo:lo + 16], rows[lo:lo + 16]
        plain = feed.batch(idx, params=par)
        affine = feed.batch(idx, params=[(*row, *IDENTITY) for row in par])
        assert torch.equal(plain["image"].view(torch.int32), affine["image"].view(torch.int32)), lo
        assert torch.equal(plain["label"], affine["label"]), lo
        assert np.array_equal(affine["image"].cpu().numpy(), want_image[lo:lo + 16])
        assert np.array_equal(affine["label"].cpu().numpy(), want_label[lo:lo + 16])
    return len(indices)


# ---- 2. proper signed permutations ----------------------------------------------------------------------------------------------------

def signed_permutations():
    """The 24 rotation matrices with entries in {0, +-1} and determinant +1, as (perm, signs, M): row a of M has signs[a] in column perm[a]."""
    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1, -1), repeat=3):
            M = np.zeros((3, 3))
            for a in range(3):
                M[a, perm[a]] = signs[a]
            if round(np.linalg.det(M)) == 1:
                out.append((perm, signs, M))
    assert len(out) == 24
    return out


def cube_store(device):
    return DeviceVolumeStore([aref.source_volume(s) for s in CUBES], device)


def check_signed_permutations(store):
    """x_a = ctr + signs[a] * (p[perm[a]] - ctr): the source reversed along every axis with a negative sign, then transposed."""
    for v, shape in enumerate(CUBES):
        image, label = aref.source_volume(shape)
        row = aref.make_row(shape, shape, (0, 0, 0), 0, 0)
        perms = signed_permutations()
        cases = [(v, row, M) for _, _, M in perms]
        got = run_cases(store, shape, cases)
        check_cases(got, cases, reference(tuple((v, row, tuple(M.reshape(-1))) for v, row, M in cases), "cubes", shape))
        for j, (perm, signs, _) in enumerate(perms):
            axes = tuple(int(a) for a in np.argsort(perm))                # out[p] = flipped[q], q[a] = p[perm[a]]
            for src, out in ((image, got[0][j, 0]), (label.astype(np.int64), got[1][j, 0])):
                flipped = np.flip(src, [a for a in range(3) if signs[a] < 0]) if any(s < 0 for s in signs) else src
                assert np.array_equal(out, np.transpose(flipped, axes)), (shape, perm, signs)


# ---- 3. dyadic zooms ------------------------------------------------------------------------------------------------------------------

def check_dyadic_zooms(store):
    """diag(1/2) and diag(2): at (5,5,5) u is an integer and u / 2 hits exact halves (half-to-even on the label, f = 0.5 on the image); at
    (8,8,8) the positions are quarter fractions.  Against the restatement, and by hand along the central depth row of the (5,5,5) cube."""
    for v, shape in enumerate(CUBES):
        row = aref.make_row(shape, shape, (0, 0, 0), 0, 0)
        cases = [(v, row, tuple(np.diag([z] * 3).reshape(-1))) for z in (0.5, 2.0)]
        got = run_cases(store, shape, cases)
        check_cases(got, cases, reference(tuple(cases), "cubes", shape))
        if shape == (5, 5, 5):
            image, label = aref.source_volume(shape)
            src, lab = image[2, 2].astype(np.float64), label[2, 2].astype(np.int64)
            # diag(1/2): x = 2 + (p - 2) / 2 = 1, 1.5, 2, 2.5, 3;  rint(1.5) = rint(2.5) = 2
            assert np.array_equal(got[0][0, 0, 2, 2], np.array([src[1], (src[1] + src[2]) / 2, src[2], (src[2] + src[3]) / 2, src[3]], dtype=np.float32))
            assert np.array_equal(got[1][0, 0, 2, 2], np.array([lab[1], lab[2], lab[2], lab[2], lab[3]]))
            # diag(2): x = 2 + 2 (p - 2) = -2, 0, 2, 4, 6: both ends lie outside the volume
            assert np.array_equal(got[0][1, 0, 2, 2], np.array([0, src[0], src[2], src[4], 0], dtype=np.float32))
            assert np.array_equal(got[1][1, 0, 2, 2], np.array([0, lab[0], lab[2], lab[4], 0]))


# ---- 4. random matrices ---------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def random_volume(v):
    return aref.big_volume(RANDOM_SOURCES[v], 60 + v)


def random_store(device):
    return DeviceVolumeStore([random_volume(v) for v in range(len(RANDOM_SOURCES))], device)


@functools.lru_cache(maxsize=None)
def random_cases(roi, plain_tail=False):
    """Six matrices per source (angles in +-0.5 rad per axis, anisotropic zoom in [0.7, 1.4]), seeded; origins at both ends and inside
    their ranges; flips, quarter turns and intensities vary unless ``plain_tail`` (the scipy cross-check)."""
    rng = np.random.RandomState(20 + roi[2])
    cases = []
    for v, shape in enumerate(RANDOM_SOURCES):
        span = [max(n - r, 0) for n, r in zip(shape, roi)]
        for q in range(6):
            M = affine_matrix(rng.uniform(-0.5, 0.5, 3), rng.uniform(0.7, 1.4, 3))
            origin = [(0, span[a], span[a] // 2)[(q + a) % 3] for a in range(3)]
            m = 6 * v + q
            mul, add = (1.0, 0.0) if plain_tail else aref.INTENSITIES[m % 3]
            row = aref.make_row(shape, roi, origin, 0 if plain_tail else (m * 3 + 1) % 8, 0 if plain_tail else m % 4, mul, add)
            cases.append((v, row, tuple(M.reshape(-1))))
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def reference(cases, volumes, roi):
    """The restatement of a tuple of cases, once: (image [N,1,*roi], label [N,1,*roi]).  ``volumes``: "cubes", "random" or "big"."""
    source = {"cubes": lambda v: aref.source_volume(CUBES[v]), "random": random_volume, "big": big_volume}[volumes]
    want = [affine_chain(*source(v), row, M, roi) for v, row, M in cases]
    return np.stack([w[0] for w in want]), np.stack([w[1] for w in want])


def check_random(store, roi):
    """Aligned outputs (the quad kernel where R2 % 4 == 0) and outputs 4 / 8 bytes off (the one-voxel kernel): both equal the restatement."""
    cases = random_cases(roi)
    want = reference(cases, "random", roi)
    for misaligned in (False, True):
        check_cases(run_cases(store, roi, list(cases), misaligned=misaligned), cases, want)
    return len(cases)


# ---- 5. non-finite voxels -------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def nonfinite_volume(v):
    """random_volume(v) with a NaN at voxel (0, 0, 0), which stands in for a tap outside the volume inside the kernel, +inf at the last
    voxel and -inf at the central one."""
    image, label = random_volume(v)
    image = image.copy()
    image[0, 0, 0] = np.nan
    image[-1, -1, -1] = np.inf
    image[tuple(n // 2 for n in image.shape)] = -np.inf
    return image, label


def nonfinite_store(device):
    return DeviceVolumeStore([nonfinite_volume(v) for v in range(len(RANDOM_SOURCES))], device)


NONFINITE_SEED = 0


@functools.lru_cache(maxsize=None)
def nonfinite_cases(roi, seed=NONFINITE_SEED):
    """Six matrices per source as in random_cases, seeded; the crop at the corner of voxel (0, 0, 0), at the opposite corner and in the
    middle in turn (the three voxels of nonfinite_volume); flips and quarter turns vary; mul = 1 and add = 0, so that a voxel without a
    tap stays +0.  The seed was chosen so that check_nonfinite's conditions hold at all three ROIS."""
    rng = np.random.RandomState(seed)
    cases = []
    for v, shape in enumerate(RANDOM_SOURCES):
        span = [max(n - r, 0) for n, r in zip(shape, roi)]
        for q in range(6):
            M = affine_matrix(rng.uniform(-0.5, 0.5, 3), rng.uniform(0.7, 1.4, 3))
            origin = [(0, span[a], span[a] // 2)[q % 3] for a in range(3)]
            m = 6 * v + q
            cases.append((v, aref.make_row(shape, roi, origin, (m * 3 + 1) % 8, m % 4, 1.0, 0.0), tuple(M.reshape(-1))))
    return tuple(cases)


def check_nonfinite(store, roi):
    """A tap outside the volume counts as 0 whatever the stand-in voxel holds; a tap inside carries its value even where its weight is 0
    (0 * inf is a NaN in the definition too).  Through icl_volume_feed_affine and icl_volume_feed_affine_origins, aligned outputs and
    outputs 4 / 8 bytes off: equal to the restatement, a NaN equal to a NaN.  What the case list must hold is asserted on the restatement
    alone: voxels with a tap outside the volume on each axis and on all three at once, a NaN carried by an inside tap at voxel (0, 0, 0), and a voxel all of whose
    eight taps are outside and whose value is +0."""
    cases = nonfinite_cases(roi)
    outside_on_axis, outside_on_all, nan_from_origin, untouched = [0, 0, 0], 0, 0, 0
    want = []
    for v, row, M in cases:
        image, label = nonfinite_volume(v)
        with np.errstate(invalid="ignore"):                              # 0 * inf and inf - inf are part of the case
            want.append(affine_chain(image, label, row, M, roi))
        fl = [np.floor(x) for x in coordinates(row, M, roi)]
        out = [[(fl[a] + bit < 0) | (fl[a] + bit > image.shape[a] - 1) for bit in (0, 1)] for a in range(3)]
        for a in range(3):
            outside_on_axis[a] += int((out[a][0] | out[a][1]).sum())
        outside_on_all += int(np.logical_and.reduce([out[a][0] | out[a][1] for a in range(3)]).sum())
        # tap (0, 0, 0) of the volume is among the eight: floor(x_a) is 0 or -1 on every axis
        at_origin = np.logical_and.reduce([(fl[a] == 0) | (fl[a] == -1) for a in range(3)])
        carried = want[-1][0][0][forwards(at_origin, row)]                # the mask is on the patch grid, the output flipped and turned
        assert np.isnan(carried).all()
        nan_from_origin += carried.size
        # every tap is outside where both taps of one axis are
        none = forwards(np.logical_or.reduce([out[a][0] & out[a][1] for a in range(3)]), row)
        value = want[-1][0][0][none]
        assert (value == 0).all() and not np.signbit(value).any()
        untouched += int(none.sum())
    print(f"roi {roi}: voxels with a tap outside per axis {outside_on_axis}, on all three {outside_on_all}; NaN from voxel (0, 0, 0) "
          f"{nan_from_origin}; no tap inside {untouched}")
    assert min(outside_on_axis) > 0 and outside_on_all > 0 and nan_from_origin > 0 and untouched > 0
    want = np.stack([w[0] for w in want]), np.stack([w[1] for w in want])
    origins = torch.tensor([c[1][3:6] for c in cases], dtype=torch.int32, device=store.device)
    for misaligned in (False, True):
        for dev_origins in (False, True):
            for lo in range(0, len(cases), 16):
                part = cases[lo:lo + 16]
                rc, image, label = raw_affine(store, roi, [c[0] for c in part], [c[1] for c in part], [c[2] for c in part], misaligned=misaligned,
                                              origins=origins[lo:lo + 16].contiguous() if dev_origins else None)
                assert rc == 0, _lib.lib().icl_last_error()
                check_cases((image.cpu().numpy(), label.cpu().numpy()[:, None]), part, (want[0][lo:lo + 16], want[1][lo:lo + 16]))
    return len(cases)


# ---- 6. mixed batch -------------------------------------------------------------------------------------------------------------------

def check_mixed_batch(store, roi=ROI_TILED):
    """17 samples, plain and affine rows alternating: two launches (16 through the affine entry, the last, plain one through
    icl_volume_feed).  Plain samples equal icl_volume_feed's, affine ones the restatement; a second run is bit-equal."""
    cases = random_cases(roi)[:17]
    want = reference(random_cases(roi), "random", roi)
    indices = [c[0] for c in cases]
    rows = [c[1] if j % 2 == 0 else (*c[1], *c[2]) for j, c in enumerate(cases)]
    feed = OnDeviceAugmentAMOS(store, roi)
    first = feed.batch(indices, params=rows)
    second = feed.batch(indices, params=rows)
    plain = feed.batch(indices, params=[c[1] for c in cases])
    assert first["image"].shape == (17, 1, *roi) and first["label"].shape == (17, 1, *roi)
    gi, gl = first["image"].cpu().numpy(), first["label"].cpu().numpy()
    for j in range(17):
        if j % 2 == 0:
            assert np.array_equal(gi[j], plain["image"][j].cpu().numpy()) and np.array_equal(gl[j], plain["label"][j].cpu().numpy()), j
            assert np.array_equal(gi[j], aref.forward_chain(*random_volume(indices[j]), cases[j][1], roi)[0]), j
        else:
            assert np.array_equal(gi[j], want[0][j]) and np.array_equal(gl[j], want[1][j]), j
    assert torch.equal(first["image"], second["image"]) and torch.equal(first["label"], second["label"])
    assert first["image"].data_ptr() != second["image"].data_ptr()


# ---- 7. device origins ----------------------------------------------------------------------------------------------------------------

def check_device_origins(device):
    """OnDeviceAugmentPosNeg with affine_prob = 1 on the pos/neg feed's small store: its batch == the host-origin entry point fed with
    the origins read back (here only) == the restatement; then an origins buffer holding -5 and n + 5 gives the clamped origins' result."""
    import posneg_feed_ref as pref
    from icl_amd.dataloaders.amos import ForegroundIndex, OnDeviceAugmentPosNeg
    store = pref.small_store(device)
    index = ForegroundIndex(store, pref.THRESHOLD)
    for roi in (ROI_QUAD, ROI_SCALAR, ROI_TILED):
        feed = OnDeviceAugmentPosNeg(store, index, roi, num_samples=2, rng=np.random.RandomState(11), flip_prob=0.5, rot_prob=0.5, affine_prob=1.0,
                                     rotate_range=0.5, zoom_range=(0.7, 1.4), zoom_isotropic=False)
        vols = [2, 0, 3, 1]
        rows = feed.draw(vols)
        assert len(rows) == 8 and all(len(r) == 27 for r in rows)
        got = feed.batch(vols, params=rows)
        sample_of = [v for v in vols for _ in range(2)]
        rc, origins = pref.raw_select(store, index, [(v, int(r[16]), int(r[17])) for v, r in zip(sample_of, rows)], roi)
        assert rc == 0
        host_rows = [(*r[:3], *[int(o) for o in origin], *r[6:16]) for r, origin in zip(rows, origins.cpu().numpy())]
        mats = [r[18:] for r in rows]
        rc, image, label = raw_affine(store, roi, sample_of, host_rows, mats)
        assert rc == 0
        assert pref.same_bits(image, got["image"]) and torch.equal(label[:, None], got["label"])
        for j, (v, row, M) in enumerate(zip(sample_of, host_rows, mats)):
            want = affine_chain(*pref.volume(v), row, M, roi)
            assert same(image[j].cpu().numpy(), want[0]) and same(label[j].cpu().numpy()[None], want[1]), (roi, j)
        # origins no select launch could leave: clamped into [0, n - s]
        v, row, M = sample_of[0], rows[0], mats[0]
        n, size = row[:3], row[6:9]
        wild = torch.tensor([[-5, n[1] + 5, n[2] + 5], [n[0] + 5, -5, -5]], dtype=torch.int32, device=store.device)
        clamped = [(0, n[1] - size[1], n[2] - size[2]), (n[0] - size[0], 0, 0)]
        rc, image, label = raw_affine(store, roi, [v, v], [row[:16]] * 2, [M] * 2, origins=wild)
        assert rc == 0
        for j in range(2):
            want = affine_chain(*pref.volume(v), (*row[:3], *clamped[j], *row[6:16]), M, roi)
            assert same(image[j].cpu().numpy(), want[0]) and same(label[j].cpu().numpy()[None], want[1]), (roi, j)


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------------

def check_refusals(store):
    """NaN, +-inf and 16.5 in M, a flag of 2, a null affine_params: -1 from the entry points with a message naming the field, nothing
    written; the same rows and a row of 20 values: ValueError from batch() before any call."""
    import pytest
    roi = ROI_SCALAR
    shape = aref.SOURCES[0]
    good = aref.make_row(shape, roi, (1, 0, 2), 3, 1, 1.0, 0.0625)
    rc, image, label = raw_affine(store, roi, [0], [good], [IDENTITY])
    assert rc == 0 and not (image == SENTINEL).any() and not (label == SENTINEL).any()

    def with_entry(e, value):
        return IDENTITY[:e] + (value,) + IDENTITY[e + 1:]

    origins = torch.zeros((2, 3), dtype=torch.int32, device=store.device)
    for dev_origins, name in ((None, "volume_feed_affine"), (origins, "volume_feed_affine_origins")):
        def refused(match, mats=(IDENTITY,), **kw):
            rc, image, label = raw_affine(store, roi, [0] * len(mats), [good] * len(mats), list(mats), origins=dev_origins, **kw)
            assert rc == -1
            with pytest.raises(RuntimeError, match=match):
                _lib.check(rc, name)
            assert (image == SENTINEL).all() and (label == SENTINEL).all()

        refused(name + ": sample 0: affine matrix entry M\\[0\\]\\[1\\] = nan is not finite", mats=[with_entry(1, float("nan"))])
        refused("sample 1: affine matrix entry M\\[2\\]\\[2\\] = inf is not finite", mats=[IDENTITY, with_entry(8, float("inf"))])
        refused("affine matrix entry M\\[1\\]\\[0\\] = -inf is not finite", mats=[with_entry(3, float("-inf"))])
        refused("affine matrix entry M\\[1\\]\\[2\\] = 16.5 outside \\[-16, 16\\]", mats=[with_entry(5, 16.5)])
        refused("affine matrix entry M\\[0\\]\\[0\\] = -16.5 outside", mats=[with_entry(0, -16.5)])
        refused("sample 1: affine flag 2 \\(must be 0 or 1\\)", mats=[IDENTITY, IDENTITY], flags=[1.0, 2.0])
        refused("affine flag 0.5", flags=[0.5])
        refused("affine_params is a null pointer", null_affine=True)
        rc, image, label = raw_affine(store, roi, [0], [good], [with_entry(4, 16.0)], origins=dev_origins)      # the bound itself is legal
        assert rc == 0 and not (image == SENTINEL).any()
    # what the siblings refuse is refused here too
    rc, image, label = raw_affine(store, roi, [0], [good[:13] + (4,) + good[14:]], [IDENTITY])
    assert rc == -1 and b"k = 4 outside 0..3" in _lib.lib().icl_last_error() and (image == SENTINEL).all()
    rc, image, label = raw_affine(store, roi, [0], [good[:3] + (-1,) + good[4:]], [IDENTITY])
    assert rc == -1 and b"crop [-1, " in _lib.lib().icl_last_error() and (label == SENTINEL).all()

    feed = OnDeviceAugmentAMOS(store, roi)
    image, label = sentinel_outputs(1, roi, store.device)
    for bad, match in (((*good, *with_entry(1, float("nan"))), "M\\[0\\]\\[1\\] = nan must be finite"),
                       ((*good, *with_entry(8, float("inf"))), "M\\[2\\]\\[2\\] = inf must be finite"),
                       ((*good, *with_entry(5, 16.5)), "M\\[1\\]\\[2\\] = 16.5 must be finite and at most 16"),
                       ((*good, 1.0, 0.0, 0.0, 0.0), "one parameter row of 16 values per index \\(25 with an affine matrix\\); row 0 has 20")):
        with pytest.raises(ValueError, match=match):
            feed.batch([0], params=[bad], out=(image, label.view(1, 1, *roi)))
        assert (image == SENTINEL).all() and (label == SENTINEL).all()


# ---- 10. the trainer's roi ------------------------------------------------------------------------------------------------------------

def big_volume(v):
    return aref.big_batch()[0][v]


@functools.lru_cache(maxsize=None)
def big_cases():
    """amos_feed_ref's batch of four at 96^3 (every flip bit, every k, non-zero shifts), each with a random M."""
    _, rows = aref.big_batch()
    rng = np.random.RandomState(96)
    return tuple((v, row, tuple(affine_matrix(rng.uniform(-0.5, 0.5, 3), rng.uniform(0.7, 1.4, 3)).reshape(-1))) for v, row in enumerate(rows))
