"""Shared restatement and checks of the simulated low resolution of the 3-D feed's intensity stage (tests/test_lowres_feed_emu.py on the
CPU emulator, tests/test_gpu_lowres_feed.py on the GPU; intensity_lowres_kernel of icl_amd/csrc/kernels/intensity.h, icl_intensity_lowres,
icl_amd/dataloaders/intensity.py).  Not a test module.

``near_ref``, ``taps_ref`` and ``lowres_ref`` restate DESIGN.md §2 "Intensity stage of the 3-D feed", low resolution, literally in numpy:
one numpy operation per rounding the definition names.  The kernel and the emulator are compared with ``lowres_ref`` BIT FOR BIT: both
sides perform the same IEEE operations (fp32 index and weight arithmetic, exact products and rounded sums in double, one rounding to
fp32), none of which goes through a library function.  The restatement itself is compared with torch's ``interpolate`` on the CPU in the
emulator's test file: indices and weights exactly, the whole chain within ``10 * 2^-24 * max|x|`` (derived there).  The rest of the
chain (noise, blur, statistics, contrast, gamma) and its bounds come from intensity_feed_ref.py.
"""
import ctypes

import numpy as np
import pytest
import torch

import intensity_feed_ref as ref
from icl_amd import _lib
from icl_amd.dataloaders.amos import ForegroundIndex, OnDeviceAugmentAMOS, OnDeviceAugmentPosNeg
from icl_amd.dataloaders.brats2019 import OnDeviceAugment, draw_rotflip_crop
from icl_amd.dataloaders.intensity import IntensityAugment, draw_intensity_params, lowres_extents

SHAPE_SCALAR = ref.SHAPE_SCALAR      # (7, 9, 10): R2 % 4 != 0, one voxel a thread
SHAPE_QUAD = ref.SHAPE_QUAD          # (8, 12, 16): one quad a thread when the batch is aligned
SHAPE_COPRIME = (9, 11, 13)
SHAPE_BIG = ref.SHAPE_BIG
CHAIN_ROI = ref.CHAIN_ROI
LOWRES_OFF = (0, 1.0, 1.0, 1.0)
F32 = np.float32


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------

def near_ref(L, R):
    """near(i), i = 0 .. L - 1: min(floor(fp32(fp32(i + 0.5) sn)), R - 1) with sn = fp32(R) / fp32(L)."""
    sn = F32(R) / F32(L)
    c = np.arange(L).astype(F32) + F32(0.5)
    p = (c * sn).astype(F32)
    return np.minimum(np.floor(p).astype(np.int64), R - 1)


def taps_ref(L, R):
    """(i0, i1, w0, w1) of every output index o = 0 .. R - 1 along one axis; the weights are fp32."""
    sl = F32(L) / F32(R)
    o = np.arange(R, dtype=np.float64)
    src = (np.float64(sl) * (o + 0.5) - 0.5).astype(F32)           # exact in double (24 x 24 bits), so ONE rounding
    src = np.where(src < 0, F32(0), src).astype(F32)
    i0 = np.minimum(src.astype(np.int64), L - 1)
    i1 = i0 + (i0 < L - 1)
    w1 = np.clip((src - i0.astype(F32)).astype(F32), F32(0), F32(1)).astype(F32)
    w0 = (F32(1) - w1).astype(F32)
    return i0, i1, w0, w1


def axis_ref(L, R):
    """(s0, s1, w0, w1) per output index: the two PATCH voxels and their weights in double."""
    i0, i1, w0, w1 = taps_ref(L, R)
    near = near_ref(L, R)
    return near[i0], near[i1], w0.astype(np.float64), w1.astype(np.float64)


def lowres_ref(x, low):
    """The sample ``x`` fp32 at the low extents ``low`` and back: along axis 2, then 1, then 0, in double, one rounding to fp32."""
    x = np.asarray(x, dtype=np.float32)
    v = x.astype(np.float64)
    for axis in (2, 1, 0):
        s0, s1, w0, w1 = axis_ref(int(low[axis]), x.shape[axis])
        shape = [1, 1, 1]
        shape[axis] = -1
        a = np.take(v, s0, axis=axis) * w0.reshape(shape)
        b = np.take(v, s1, axis=axis) * w1.reshape(shape)
        v = a + b
    return v.astype(np.float32)


def torch_chain(x, low):
    """What batchgeneratorsv2's SimulateLowResolutionTransform is made of, on the CPU."""
    import torch.nn.functional as F
    t = torch.as_tensor(np.array(x, dtype=np.float32))[None, None]
    down = F.interpolate(t, size=tuple(int(v) for v in low), mode="nearest-exact")
    return F.interpolate(down, size=tuple(x.shape), mode="trilinear", align_corners=False)[0, 0].numpy()


def zooms_for(shape, low):
    """Zooms that ``lowres_extents`` turns into exactly ``low``."""
    z = tuple(float(l) / float(r) for l, r in zip(low, shape))
    assert lowres_extents(shape, z) == tuple(low)
    return z


def row(lowres=None, **kw):
    """A row of 15: ``intensity_feed_ref.row(**kw)``, then (flag, z0, z1, z2); ``lowres`` is the three zooms or None."""
    return ref.row(**kw) + (LOWRES_OFF if lowres is None else (1, *[float(z) for z in lowres]))


def low_of(shape, r):
    """The low extents of a row, ``shape`` itself where the row does not carry the transform."""
    return lowres_extents(shape, r[12:15]) if len(r) == 15 and r[11] else tuple(shape)


def chain_ref(x, r):
    """The whole stage on one sample: noise, blur, LOW RESOLUTION, statistics, contrast, gamma: (y, stats or None, per-voxel slack).
    As intensity_feed_ref.chain_ref, with one step more.  Low resolution is a convex combination of the sample's voxels rounded once,
    so noise's slack (at most ``e`` on every input) becomes at most ``max e`` plus one rounding on either side, ``2^-23 |want|``; without
    noise the slack stays 0 and the comparison exact."""
    x = np.asarray(x, dtype=np.float32)
    slack = np.zeros(x.shape, dtype=np.float64)
    if r[0]:
        x, n = ref.noise_ref(x, r[1], r[2], r[3])
        slack = 2.0 ** -23 * (np.abs(n).astype(np.float64) + np.abs(x))
    if r[4]:
        x = ref.blur_ref(x, r[5])
    low = low_of(x.shape, r)
    if low != x.shape:
        x = lowres_ref(x, low)
        if r[0]:
            slack = slack.max() + 2.0 ** -23 * np.abs(x).astype(np.float64)
    stats = None
    if r[6] or r[8]:
        stats = ref.stats_ref(x)
        x, mag = ref.point_ref(x, r, stats)
        if mag is not None:
            slack = np.full(x.shape, float(np.spacing(np.float32(mag))), dtype=np.float64)
    return x, stats, slack


# ---- running the stage ------------------------------------------------------------------------------------------------------------------

def run_stage(device, samples, rows, misaligned=False):
    """``IntensityAugment.apply`` on a batch built from ``samples``, as intensity_feed_ref.run_stage, with the stage's scratch buffer
    full of NaN beforehand: (result [B, *shape], stats [B, 4] or None, the stage)."""
    shape = samples[0].shape
    n, per = len(samples), int(np.prod(shape))
    stage = IntensityAugment(shape)
    stage._buffer("_scratch", 16 * per, torch.float32, torch.device(device)).fill_(float("nan"))
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
    return out.cpu().numpy()[:, 0], (None if stage.stats is None else stage.stats.cpu().numpy()), stage


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


# ---- the checks, shared by the emulator and the GPU ----------------------------------------------------------------------------------------

def sample_cases():
    """(shape, misaligned, [low extents of sample 0, of sample 1]): exactly half, one axis at 1 (i1 = i0 everywhere), one axis at R
    (left alone), and coprime extents."""
    cases = []
    for shape, misaligned in ((SHAPE_SCALAR, False), (SHAPE_QUAD, False), (SHAPE_QUAD, True)):
        half = lowres_extents(shape, (0.5, 0.5, 0.5))
        r0, r1, r2 = shape
        cases.append((shape, misaligned, [half, (r0 - 2, 1, r2 - 3)]))
        cases.append((shape, misaligned, [(r0 - 3, r1, r2 // 2 + 1), (1, r1 - 1, r2)]))
        cases.append((shape, misaligned, [(r0, r1, 1), (r0 - 1, r1 - 5, r2 - 1)]))
    cases.append((SHAPE_COPRIME, False, [(5, 9, 7), (7, 4, 11)]))
    assert lowres_extents(SHAPE_QUAD, (0.5, 0.5, 0.5)) == (4, 6, 8) and lowres_extents(SHAPE_SCALAR, (0.5, 0.5, 0.5)) == (4, 4, 5)
    return cases


def check_samples(device):
    """Bit-equal to the restatement, two samples a launch, on the scalar path, the quad path and the quad shape on a misaligned batch."""
    total = 0
    for shape, misaligned, lows in sample_cases():
        samples = [ref.patch(shape, 101 + j) for j in range(len(lows))]
        rows = [row(lowres=zooms_for(shape, low)) for low in lows]
        got, stats, _ = run_stage(device, samples, rows, misaligned)
        for j, low in enumerate(lows):
            want = lowres_ref(samples[j], low)
            assert same_bits(got[j], want), (shape, misaligned, low, ref.differing(got[j], want))
            assert want.min() >= samples[j].min() and want.max() <= samples[j].max(), "a convex combination left the sample's range"
            total += 1
        assert stats is not None and not stats.any(), "low resolution alone takes no statistics"
    # an axis at R is left alone: every plane across it is what the other two axes make of that plane by itself
    shape = SHAPE_QUAD
    x = ref.patch(shape, 111)
    got, _, _ = run_stage(device, [x], [row(lowres=zooms_for(shape, (shape[0], 5, 7)))])
    for k in range(shape[0]):
        plane = lowres_ref(x[k:k + 1], (1, 5, 7))
        assert same_bits(got[0][k:k + 1], plane), k
    return total


def check_mixed_batch(device):
    """Samples that did not draw the transform come back bit-identical to the plain feed; nothing of the (NaN-filled) scratch buffer
    reaches them or anybody else; rows of 11 and of 15 may share a batch."""
    store = ref.loader_store(device)
    indices = [0, 1, 2, 1, 0]
    geo = OnDeviceAugmentAMOS(store, CHAIN_ROI, rng=np.random.RandomState(2), rot_prob=0.0).draw(indices)
    base = OnDeviceAugmentAMOS(store, CHAIN_ROI, rot_prob=0.0).batch(indices, params=geo)["image"].cpu().numpy()[:, 0]
    rows = [row(lowres=(0.5, 0.5, 0.5)), row(), ref.row(), row(lowres=(1.0, 1.0, 1.0)), row(lowres=(0.7, 1.0, 0.4), contrast=1.2)]
    stage = IntensityAugment(CHAIN_ROI)
    stage._buffer("_scratch", 16 * int(np.prod(CHAIN_ROI)), torch.float32, torch.device(device)).fill_(float("nan"))
    mixed = OnDeviceAugmentAMOS(store, CHAIN_ROI, rot_prob=0.0, intensity=stage).batch(indices, params=geo, intensity_params=rows)
    mixed = mixed["image"].cpu().numpy()[:, 0]
    assert np.isfinite(mixed).all()
    for j in (1, 2, 3):
        assert same_bits(mixed[j], base[j]), j
    assert same_bits(mixed[0], lowres_ref(base[0], (4, 4, 6)))
    want, want_stats, _ = chain_ref(base[4], rows[4])
    assert same_bits(mixed[4], want) and ref.differing(mixed[4], base[4]) > 0
    stats = stage.stats.cpu().numpy()
    assert not stats[:4].any() and tuple(stats[4, :3]) == tuple(float(v) for v in want_stats)
    # the plain binding, all flags 0: returns 0 and launches nothing (the scratch buffer stays as it is)
    x = torch.as_tensor(base[:2].copy()).to(device)
    scratch = torch.full_like(x, 7.0)
    p = (ctypes.c_int32 * 8)(0, 4, 4, 6, 0, *CHAIN_ROI)
    assert _lib.lib().icl_intensity_lowres(x.data_ptr(), scratch.data_ptr(), p, 2, *CHAIN_ROI, None) == 0
    p = (ctypes.c_int32 * 8)(1, *CHAIN_ROI, 0, 1, 1, 1)                        # on, but the identity
    assert _lib.lib().icl_intensity_lowres(x.data_ptr(), scratch.data_ptr(), p, 2, *CHAIN_ROI, None) == 0
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()
    assert same_bits(x.cpu().numpy(), base[:2]) and bool((scratch == 7.0).all())


ALL_ON = dict(ref.ALL_ON, lowres_prob=1.0, lowres_zoom=(0.3, 0.9), lowres_per_axis=True)


def chain_rows():
    """17 rows of 15: intensity_feed_ref.chain_rows() (every transform on in the first nine, then each alone, none, and pairs) with low
    resolution on in most of them: per-axis zooms, a shared zoom, one axis left alone, one axis at 1; four rows without it."""
    base = ref.chain_rows()
    rng = np.random.RandomState(12)
    lows = [tuple(rng.uniform(0.3, 0.9, 3)) for _ in range(9)]
    lows += [(0.5, 0.5, 0.5), None, (0.6, 1.0, 0.6), (0.05, 0.7, 0.7), (0.45, 0.45, 0.45), None, (1.0, 1.0, 0.5), None]
    rows = [b + (LOWRES_OFF if z is None else (1, *[float(v) for v in z])) for b, z in zip(base, lows)]
    assert len(rows) == 17 and all(len(r) == 15 for r in rows) and lowres_extents(CHAIN_ROI, lows[12]) == (1, 6, 8)
    return rows


def compare_with_chain(plain, got, stats, rows, what):
    """``got`` == the restatement applied to the plain feed's output: exact for a sample without noise and gamma, else within the
    slack; ``stats`` are the statistics of the low-resolution sample."""
    slack_used = 0
    for j, r in enumerate(rows):
        want, want_stats, slack = chain_ref(plain[j], r)
        if not (r[0] or r[8]):
            assert same_bits(got[j], want), (what, j, r, ref.differing(got[j], want))
        else:
            diff = np.abs(got[j].astype(np.float64) - want.astype(np.float64))
            assert (diff <= slack).all(), (what, j, r, float(diff.max()))
            slack_used += ref.differing(got[j], want)
        if want_stats is None:
            assert not stats[j].any(), (what, j)
        elif not r[0]:                                             # no noise: the statistics' input is exact, and so are they
            assert same_bits(stats[j, :3], np.array(want_stats, dtype=np.float32)), (what, j, stats[j], want_stats)
        else:
            # noise: every input of the statistics is within an fp32 ulp of the restatement's (2^-23 of the largest magnitude), and so
            # are min, max and the mean, the mean with its own rounding (2^-24) on top
            bound = 2.0 ** -22 * float(max(abs(want_stats[0]), abs(want_stats[1])))
            assert np.abs(stats[j, :3].astype(np.float64) - np.array(want_stats, dtype=np.float64)).max() <= bound, (what, j)
    print(f"{what}: {slack_used} voxels differ at all over {len(rows)} samples")


def check_chain_amos(device):
    """One batch of 17 through OnDeviceAugmentAMOS(intensity=...) with every transform on: two chunks."""
    store = ref.loader_store(device)
    indices = [j % len(ref.STORE_SHAPES) for j in range(17)]
    geo = OnDeviceAugmentAMOS(store, CHAIN_ROI, rng=np.random.RandomState(3), flip_prob=0.5, rot_prob=0.0).draw(indices)
    plain = OnDeviceAugmentAMOS(store, CHAIN_ROI, rot_prob=0.0).batch(indices, params=geo)
    feed = OnDeviceAugmentAMOS(store, CHAIN_ROI, rot_prob=0.0, intensity=IntensityAugment(CHAIN_ROI, **ALL_ON))
    rows = chain_rows()
    got = feed.batch(indices, params=geo, intensity_params=rows)
    assert torch.equal(got["label"], plain["label"])
    first = got["image"].cpu().numpy()[:, 0]
    assert tuple(feed.intensity.stats.shape) == (17, 4)
    compare_with_chain(plain["image"].cpu().numpy()[:, 0], first, feed.intensity.stats.cpu().numpy(), rows, "AMOS feed")
    again = feed.batch(indices, params=geo, intensity_params=rows)["image"].cpu().numpy()[:, 0]
    assert same_bits(first, again)
    # and with rows the stage draws itself: 15 values each, all carrying the transform
    feed.intensity.rng = np.random.RandomState(21)
    drawn = feed.intensity.draw(3)
    assert all(len(r) == 15 and r[11] == 1 and all(0.3 <= z <= 0.9 for z in r[12:]) for r in drawn)
    got = feed.batch(indices[:3], params=geo[:3], intensity_params=drawn)
    compare_with_chain(plain["image"].cpu().numpy()[:3, 0], got["image"].cpu().numpy()[:, 0], feed.intensity.stats.cpu().numpy(), drawn,
                       "AMOS feed, drawn rows")


def check_chain_other_stores(device):
    """The BraTS feed and the pos/neg feed with the stage, roi (8, 8, 12)."""
    store = ref.loader_store(device)
    np.random.seed(9)
    geo = [draw_rotflip_crop(store.images[i].shape, CHAIN_ROI) for i in (0, 1, 2)]
    rows = chain_rows()[:2] + [row(lowres=(0.5, 0.8, 0.5), blur=1.0, contrast=0.9)]
    plain = OnDeviceAugment(store, CHAIN_ROI).batch([0, 1, 2], params=geo)
    stage = IntensityAugment(CHAIN_ROI, **ALL_ON)
    got = OnDeviceAugment(store, CHAIN_ROI, intensity=stage).batch([0, 1, 2], params=geo, intensity_params=rows)
    assert torch.equal(got["label"], plain["label"]) and got["image"].shape == (3, 1, *CHAIN_ROI)
    compare_with_chain(plain["image"].cpu().numpy()[:, 0], got["image"].cpu().numpy()[:, 0], stage.stats.cpu().numpy(), rows, "BraTS feed")
    index = ForegroundIndex(store)
    kw = dict(num_samples=2, rot_prob=0.0)
    geo = OnDeviceAugmentPosNeg(store, index, CHAIN_ROI, rng=np.random.RandomState(4), **kw).draw([2, 0])
    rows = chain_rows()[7:11]
    plain = OnDeviceAugmentPosNeg(store, index, CHAIN_ROI, **kw).batch([2, 0], params=geo)
    stage = IntensityAugment(CHAIN_ROI, **ALL_ON)
    got = OnDeviceAugmentPosNeg(store, index, CHAIN_ROI, intensity=stage, **kw).batch([2, 0], params=geo, intensity_params=rows)
    assert torch.equal(got["label"], plain["label"]) and got["image"].shape == (4, 1, *CHAIN_ROI)
    compare_with_chain(plain["image"].cpu().numpy()[:, 0], got["image"].cpu().numpy()[:, 0], stage.stats.cpu().numpy(), rows, "pos/neg feed")


def check_off_is_off(device):
    """A stage with lowres_prob = 0 (its other low-resolution keywords set) gives the plain feed's batches and leaves the generator
    where the plain feed leaves it, for the seeds of intensity_feed_ref.check_off_is_off; rows that are all off launch nothing."""
    ref.check_off_is_off(device)
    store = ref.loader_store(device)
    indices = [0, 1, 2, 1]
    off = dict(lowres_prob=0.0, lowres_zoom=(0.25, 0.5), lowres_per_axis=True, lowres_axes=(0, 2))
    a, b = np.random.RandomState(17), np.random.RandomState(17)
    plain = OnDeviceAugmentAMOS(store, CHAIN_ROI, rng=a, rot_prob=0.0).batch(indices)
    stage = IntensityAugment(CHAIN_ROI, rng=b, **off)
    assert not stage.enabled and stage.draw(2) == [ref.OFF_ROW] * 2
    got = OnDeviceAugmentAMOS(store, CHAIN_ROI, rng=b, rot_prob=0.0, intensity=stage).batch(indices)
    assert torch.equal(plain["image"], got["image"]) and torch.equal(plain["label"], got["label"]) and a.rand() == b.rand()
    index = ForegroundIndex(store)
    a, b = np.random.RandomState(18), np.random.RandomState(18)
    plain_pn = OnDeviceAugmentPosNeg(store, index, CHAIN_ROI, num_samples=2, rng=a, rot_prob=0.0).batch([0, 2])
    got_pn = OnDeviceAugmentPosNeg(store, index, CHAIN_ROI, num_samples=2, rng=b, rot_prob=0.0,
                                   intensity=IntensityAugment(CHAIN_ROI, rng=b, **off)).batch([0, 2])
    assert torch.equal(plain_pn["image"], got_pn["image"]) and a.rand() == b.rand()
    np.random.seed(19)
    plain_b = OnDeviceAugment(store, (8, 8, 8)).batch([0, 1])
    state = np.random.get_state()[1].copy()
    np.random.seed(19)
    got_b = OnDeviceAugment(store, (8, 8, 8), intensity=IntensityAugment((8, 8, 8), **off)).batch([0, 1])
    assert torch.equal(plain_b["image"], got_b["image"]) and np.array_equal(state, np.random.get_state()[1])
    # a stage with the other four transforms on draws the rows it drew before low resolution existed
    kw = dict(ref.ALL_ON)
    assert draw_intensity_params(np.random.RandomState(5), 9, **kw, **off) == draw_intensity_params(np.random.RandomState(5), 9, **kw)
    # all-off rows of 15, and rows whose zooms round to the patch itself: nothing is launched, no buffer is made
    x = ref.patch(CHAIN_ROI, 7)
    for rows in ([row(), row()], [row(lowres=(1.0, 1.0, 1.0)), row(lowres=(0.97, 0.95, 0.97))]):
        stage = IntensityAugment(CHAIN_ROI)
        image = torch.as_tensor(np.stack([x, x])[:, None]).to(device)
        assert stage.apply(image, rows) is image
        assert stage.stats is None and stage._scratch is None and stage._ws is None
        assert same_bits(image.cpu().numpy()[0, 0], x)
    assert lowres_extents(CHAIN_ROI, (0.97, 0.95, 0.97)) == CHAIN_ROI


def check_refusals(device):
    """Every refusal of icl_intensity_lowres returns -1 with its message and writes nothing: the batch and the scratch buffer are
    compared afterwards."""
    L = _lib.lib()
    shape = (8, 12, 16)
    x = torch.as_tensor(np.stack([ref.patch(shape, 51), ref.patch(shape, 52)])).to(device).contiguous()
    before = x.clone()
    scratch = torch.full_like(x, 3.0)
    I = lambda *v: (ctypes.c_int32 * len(v))(*v)                               # noqa: E731

    def refused(rc, text):
        assert rc == -1, (rc, text)
        msg = L.icl_last_error().decode()
        assert "intensity_lowres" in msg and text in msg, (text, msg)

    ok = (1, 4, 6, 8)
    call = lambda p, b=2, ptr=x.data_ptr(), sc=scratch.data_ptr(), r=shape: L.icl_intensity_lowres(ptr, sc, p, b, *r, None)   # noqa: E731
    refused(call(None), "null pointer")
    refused(call(I(*ok * 2), ptr=None), "null pointer")
    refused(call(I(*ok * 2), sc=None), "null pointer")
    refused(call(I(*ok * 2), sc=x.data_ptr()), "scratch")
    refused(call(I(*ok * 2), b=0), "batch")
    refused(call(I(*ok * 2), b=17), "batch")
    refused(call(I(*ok * 2), r=(0, 12, 16)), "extents")
    refused(call(I(*ok * 2), r=(8, -1, 16)), "extents")
    refused(call(I(*ok * 2), r=(2048, 2048, 1024)), "2^31")
    for bad, text in (((2, 4, 6, 8), "flag"), ((-1, 4, 6, 8), "flag"), ((1, 0, 6, 8), "low extent"), ((1, 9, 6, 8), "low extent"),
                      ((1, 4, 13, 8), "low extent"), ((1, 4, 6, 17), "low extent"), ((1, 4, 6, -3), "low extent"),
                      ((0, 4, 6, 0), "low extent"), ((0, 4, 6, 2 ** 31 - 1), "low extent")):
        refused(call(I(*ok, *bad)), text)
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()
    assert torch.equal(x, before) and bool((scratch == 3.0).all())
    # what apply refuses before anything travels
    stage = IntensityAugment(shape)
    image = before.clone().view(2, 1, *shape)
    good = row(lowres=(0.5, 0.5, 0.5))
    for bad, match in ((good[:14], "11 expected"), (good + (1,), "11 expected"), (good[:12] + (0.0, 0.5, 0.5), "zoom"), (good[:12] + (0.5, 1.5, 0.5), "zoom"),
                       (good[:12] + (0.5, 0.5, float("nan")), "zoom"), (good[:11] + (2, 0.5, 0.5, 0.5), "flag"), (good[:12] + (-0.5, 0.5, 0.5), "zoom")):
        with pytest.raises(ValueError, match=match):
            stage.apply(image, [good, bad])
    assert torch.equal(image.view_as(before), before) and stage._scratch is None
