"""Intensity stage of the 3-D device feed: Gaussian noise, Gaussian blur, simulated low resolution, contrast and gamma on the patch.

The geometric feeds (``OnDeviceAugment``, ``OnDeviceAugmentAMOS``, ``OnDeviceAugmentPosNeg``) write the image batch ``[B,1,R0,R1,R2]``
fp32 (``OnDeviceAugment`` over a multi-modal store: ``[B,C,R0,R1,R2]``, every channel a patch of its own to this stage);``IntensityAugment.apply`` then acts on it IN PLACE, on the same stream, without a word from the host.  Labels are untouched.  The
transforms stand for nnU-Net's ``GaussianNoiseTransform``, ``GaussianBlurTransform``, ``SimulateLowResolutionTransform``,
``ContrastAugmentationTransform`` (with ``preserve_range``) and ``GammaTransform`` (with ``invert_image``), MONAI's
``RandGaussianNoised``, ``RandGaussianSmoothd`` and
``RandAdjustContrastd``, and the reference's own ``RandomNoise`` (``dataloaders/brats2019.py:150-161``, clipped Gaussian noise).  Per
sample, in this order, each drawn independently and OFF by default:

1. noise: ``x += n``, ``n ~ N(0, sigma^2)``, optionally clipped to ``+-clip * sigma``;
2. blur: ``scipy.ndimage.gaussian_filter(x, sigma, mode="reflect", truncate=4.0)``;
3. low resolution: ``interpolate(interpolate(x, size=L, mode="nearest-exact"), size=R, mode="trilinear")`` with the low extents
   ``L = lowres_extents(R, zooms)``; nnU-Net applies it behind contrast, here it stands BEFORE the statistics, so that one statistics
   pass serves contrast and gamma (DESIGN.md says why that is deliberate);
4. contrast: ``(x - mean) * f + mean`` clipped to the sample's ``[min, max]``;
5. gamma: ``((x - mn) / (mx - mn + 1e-7)) ** g * (mx - mn) + mn``, on ``-x`` and negated again with ``invert``.

The definition, rounding by rounding, is in DESIGN.md §2 "Intensity stage of the 3-D feed"; ``tests/intensity_feed_ref.py`` restates it
in numpy (``tests/lowres_feed_ref.py`` for low resolution, which is also compared with torch's own ``interpolate`` on the CPU).  Blur, low
resolution, statistics and contrast equal the restatement bit for bit; noise and gamma go through ``log`` / ``cos`` / ``pow`` in
double and may differ from numpy's only where a double result sits on an fp32 rounding tie.  With every probability 0 nothing is drawn
and nothing is launched.  **Parity with MONAI's and nnU-Net's own code is unpinned**: neither is installed where this package is built
and tested; MONAI's smoothing kernel, for one, is truncated and normalised differently from scipy's.  For low resolution what is pinned
is the ``interpolate`` chain that batchgeneratorsv2's class is made of, not the class.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _lib

INTENSITY_MAX_BATCH = 16            # samples per launch (kFeedMaxBatch)
BLUR_MAX_RADIUS = 12                # kBlurMaxRadius: r = int(4 sigma + 0.5) <= 12 covers sigma <= 3
BLUR_MAX_LINE = 4096                # kBlurLineFloats: the largest extent of the contiguous axis the blur takes
INTENSITY_WS_DOUBLES = 16 * 64 * 3  # doubles of scratch icl_intensity_stats takes (kFeedMaxBatch * kIntensityStatBlocks * 3)
ROW_LENGTH = 11
LOWRES_ROW_LENGTH = 15              # a row that carries low resolution: the 11, then (lowres, z0, z1, z2)

# a row of draw_intensity_params: (noise, seed, noise sigma, noise clip, blur, blur sigma, contrast, f, gamma, g, invert)
_NOISE, _SEED, _NSIGMA, _NCLIP, _BLUR, _BSIGMA, _CONTRAST, _F, _GAMMA, _G, _INVERT = range(ROW_LENGTH)
_LOWRES, _Z0 = 11, 12
OFF_ROW = (0, 0, 1.0, 0.0, 0, 1.0, 0, 1.0, 0, 1.0, 0)      # no transform; every field legal for the C ABI


def blur_radius(sigma: float) -> int:
    """scipy's radius for ``truncate=4.0``: ``int(4 * sigma + 0.5)``."""
    return int(4.0 * float(sigma) + 0.5)


def blur_weights(sigma: float) -> np.ndarray:
    """``w_0 .. w_r`` of scipy's ``_gaussian_kernel1d(sigma, 0, r)`` (the kernel is symmetric): ``exp(-0.5 k^2 / sigma^2)`` for
    ``k = -r .. r``, divided by their sum, in double, with numpy's ``exp`` and ``sum`` — the very operations scipy performs."""
    sigma = float(sigma)
    r = blur_radius(sigma)
    x = np.arange(-r, r + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    phi = phi / phi.sum()
    return phi[r:].copy()


def lowres_extents(roi: Sequence[int], zooms: Sequence[float]) -> Tuple[int, ...]:
    """The low extents of a patch of ``roi`` under ``zooms``: ``max(1, int(np.rint(R_a * z_a)))`` per axis, the product in double and
    ties to even, as Python's ``round`` in nnU-Net."""
    if len(roi) != len(zooms):
        raise ValueError(f"lowres_extents: {len(roi)} extents, {len(zooms)} zooms")
    return tuple(max(1, int(np.rint(float(r) * float(z)))) for r, z in zip(roi, zooms))


def _probability(name: str, p) -> float:
    p = float(p)
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"{name} {p!r} must be in [0, 1]")
    return p


def _sigma_range(name: str, v) -> Tuple[float, ...]:
    """One finite positive number (no draw) or ``(lo, hi)`` with ``0 < lo <= hi`` (one uniform draw per sample)."""
    a = np.asarray(v, dtype=np.float64).reshape(-1)
    if a.size not in (1, 2) or not np.isfinite(a).all() or (a <= 0).any() or (a.size == 2 and a[0] > a[1]):
        raise ValueError(f"{name} {v!r} must be a finite positive number or (lo, hi) with 0 < lo <= hi")
    return tuple(float(x) for x in a)


def _factor_range(name: str, v) -> Tuple[float, float]:
    a = np.asarray(v, dtype=np.float64).reshape(-1)
    if a.size != 2 or not np.isfinite(a).all() or not 0.0 < a[0] <= a[1]:
        raise ValueError(f"{name} {v!r} must be (lo, hi) with 0 < lo <= hi")
    return float(a[0]), float(a[1])


def _zoom_range(name: str, v) -> Tuple[float, float]:
    a = np.asarray(v, dtype=np.float64).reshape(-1)
    if a.size != 2 or not np.isfinite(a).all() or not 0.0 < a[0] <= a[1] <= 1.0:
        raise ValueError(f"{name} {v!r} must be (lo, hi) with 0 < lo <= hi <= 1")
    return float(a[0]), float(a[1])


def _axes(name: str, v) -> Tuple[int, ...]:
    try:
        axes = [int(a) for a in v]
        ok = len(axes) >= 1 and len(set(axes)) == len(axes) and all(a in (0, 1, 2) and a == b for a, b in zip(axes, v))
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"{name} {v!r} must name one to three distinct axes out of 0, 1, 2")
    return tuple(sorted(axes))


def _intensity_arguments(noise_prob=0.0, noise_sigma=0.1, noise_clip=0.0, blur_prob=0.0, blur_sigma=(0.5, 1.0), contrast_prob=0.0,
                         contrast_range=(0.75, 1.25), gamma_prob=0.0, gamma_range=(0.7, 1.5), invert_prob=0.0, lowres_prob=0.0,
                         lowres_zoom=(0.5, 1.0), lowres_per_axis=False, lowres_axes=(0, 1, 2)) -> tuple:
    """The keywords of ``draw_intensity_params``, checked, in ``_draw_row``'s order; an unknown keyword is a ``TypeError``."""
    clip = float(noise_clip)
    if not np.isfinite(clip) or clip < 0:
        raise ValueError(f"noise_clip {noise_clip!r} must be finite and non-negative (0: no clipping)")
    blur = _sigma_range("blur_sigma", blur_sigma)
    if blur_radius(blur[-1]) > BLUR_MAX_RADIUS:
        raise ValueError(f"blur_sigma {blur_sigma!r}: the radius int(4 sigma + 0.5) = {blur_radius(blur[-1])} exceeds {BLUR_MAX_RADIUS}")
    return (_probability("noise_prob", noise_prob), _sigma_range("noise_sigma", noise_sigma), clip, _probability("blur_prob", blur_prob), blur,
            _probability("contrast_prob", contrast_prob), _factor_range("contrast_range", contrast_range),
            _probability("gamma_prob", gamma_prob), _factor_range("gamma_range", gamma_range), _probability("invert_prob", invert_prob),
            _probability("lowres_prob", lowres_prob), _zoom_range("lowres_zoom", lowres_zoom), bool(lowres_per_axis),
            _axes("lowres_axes", lowres_axes))


def _draw_sigma(rng, spec) -> float:
    return spec[0] if len(spec) == 1 else float(rng.uniform(spec[0], spec[1]))


def _draw_factor(rng, lo: float, hi: float) -> float:
    """nnU-Net's draw of a contrast factor or a gamma: ``rng.rand() < 0.5 and lo < 1`` chooses ``uniform(lo, 1)``, otherwise
    ``uniform(max(lo, 1), hi)``."""
    if rng.rand() < 0.5 and lo < 1:
        return float(rng.uniform(lo, 1))
    return float(rng.uniform(max(lo, 1), hi))


def _draw_row(rng, noise_prob, noise_sigma, noise_clip, blur_prob, blur_sigma, contrast_prob, contrast_range, gamma_prob, gamma_range,
              invert_prob, lowres_prob=0.0, lowres_zoom=(0.5, 1.0), lowres_per_axis=False, lowres_axes=(0, 1, 2)) -> tuple:
    row = list(OFF_ROW)
    if noise_prob > 0 and rng.rand() < noise_prob:
        row[_NOISE] = 1
        row[_SEED] = int(rng.randint(0, 2 ** 32))
        row[_NSIGMA] = _draw_sigma(rng, noise_sigma)
        row[_NCLIP] = noise_clip
    if blur_prob > 0 and rng.rand() < blur_prob:
        row[_BLUR] = 1
        row[_BSIGMA] = _draw_sigma(rng, blur_sigma)
    lowres = None
    if lowres_prob > 0:                                  # drawn here, between blur and contrast; kept behind the 11 fields
        lowres = [0, 1.0, 1.0, 1.0]
        if rng.rand() < lowres_prob:
            lowres[0] = 1
            if lowres_per_axis:
                for a in lowres_axes:
                    lowres[1 + a] = float(rng.uniform(*lowres_zoom))
            else:
                z = float(rng.uniform(*lowres_zoom))
                for a in lowres_axes:
                    lowres[1 + a] = z
    if contrast_prob > 0 and rng.rand() < contrast_prob:
        row[_CONTRAST] = 1
        row[_F] = float(np.float32(_draw_factor(rng, *contrast_range)))
    if gamma_prob > 0 and rng.rand() < gamma_prob:
        row[_GAMMA] = 1
        if invert_prob > 0:
            row[_INVERT] = int(rng.rand() < invert_prob)
        row[_G] = _draw_factor(rng, *gamma_range)
    if lowres is not None:
        row += lowres
    return tuple(row)


def draw_intensity_params(rng=np.random, n: int = 1, **keywords) -> List[tuple]:
    """The random draws of the intensity stage for ``n`` samples from ``rng`` (``np.random`` or a ``RandomState``): one row per sample,
    sample after sample, and for each sample in this fixed order (a transform whose probability is 0 draws NOTHING):

    1. noise (``noise_prob > 0``): ``rng.rand() < noise_prob``; ONLY IF true, ``seed = rng.randint(0, 2**32)``, then
       ``sigma = rng.uniform(lo, hi)`` ONLY IF ``noise_sigma`` is a pair (a single number is used as it is, without a draw);
    2. blur (``blur_prob > 0``): ``rng.rand() < blur_prob``; ONLY IF true, ``sigma = rng.uniform(lo, hi)`` ONLY IF ``blur_sigma`` is a pair;
    3. low resolution (``lowres_prob > 0``): ``rng.rand() < lowres_prob``; ONLY IF true, the zoom: ONE ``rng.uniform(lo, hi)`` shared by
       the axes of ``lowres_axes``, or with ``lowres_per_axis`` one ``rng.uniform(lo, hi)`` per listed axis in increasing axis order;
       an axis that is not listed gets the zoom 1;
    4. contrast (``contrast_prob > 0``): ``rng.rand() < contrast_prob``; ONLY IF true, nnU-Net's factor: ``rng.rand() < 0.5 and lo < 1``
       chooses ``rng.uniform(lo, 1)``, otherwise ``rng.uniform(max(lo, 1), hi)``; the factor is rounded to fp32;
    5. gamma (``gamma_prob > 0``): ``rng.rand() < gamma_prob``; ONLY IF true, ``invert = rng.rand() < invert_prob`` ONLY IF
       ``invert_prob > 0``, then ``g`` from ``gamma_range`` as the contrast factor is drawn (kept in double).

    Returns ``n`` rows of 11 values ``(noise, seed, noise sigma, noise clip, blur, blur sigma, contrast, f, gamma, g, invert)``: the
    five flags are 0 or 1, and the fields of a transform that was not drawn hold neutral legal values (``OFF_ROW``).  Keywords and
    defaults: ``noise_prob=0, noise_sigma=0.1, noise_clip=0`` (0: no clipping; the reference's ``RandomNoise`` is ``noise_sigma=0.1,
    noise_clip=2``), ``blur_prob=0, blur_sigma=(0.5, 1.0), contrast_prob=0, contrast_range=(0.75, 1.25), gamma_prob=0,
    gamma_range=(0.7, 1.5), invert_prob=0``.

    While ``lowres_prob`` is 0 the rows are these 11 values.  With ``lowres_prob > 0`` EVERY row has 15: the 11, then ``(lowres, z0, z1,
    z2)``, the flag and the zoom per axis in (0, 1] (1, 1, 1 where the transform was not drawn); ``lowres_extents(roi, (z0, z1, z2))``
    gives the low extents.  Keywords: ``lowres_prob=0, lowres_zoom=(0.5, 1.0)`` (``0 < lo <= hi <= 1``), ``lowres_per_axis=False,
    lowres_axes=(0, 1, 2)`` (nnU-Net's ``ignore_axes`` are the axes left out)."""
    args = _intensity_arguments(**keywords)
    n = int(n)
    if n < 0:
        raise ValueError(f"draw_intensity_params: n = {n}")
    return [_draw_row(rng, *args) for _ in range(n)]


def _checked_rows(params, n: int) -> List[tuple]:
    """Rows as ``apply`` takes them: ``n`` rows of 11 values, or of 15 with low resolution, flags 0 or 1, every field what the C ABI
    accepts."""
    if len(params) != n:
        raise ValueError(f"IntensityAugment.apply: one intensity row of {ROW_LENGTH} values per sample ({n}), got {len(params)}")
    rows = []
    for j, row in enumerate(params):
        if len(row) not in (ROW_LENGTH, LOWRES_ROW_LENGTH):
            raise ValueError(f"IntensityAugment.apply: intensity row {j} has {len(row)} values, {ROW_LENGTH} expected "
                             f"(or {LOWRES_ROW_LENGTH} with low resolution)")
        for k in (_NOISE, _BLUR, _CONTRAST, _GAMMA, _INVERT) + ((_LOWRES,) if len(row) == LOWRES_ROW_LENGTH else ()):
            if row[k] not in (0, 1):
                raise ValueError(f"IntensityAugment.apply: intensity row {j}: flag {row[k]!r} in field {k} (must be 0 or 1)")
        seed = row[_SEED]
        if int(seed) != seed or not 0 <= int(seed) < 2 ** 32:
            raise ValueError(f"IntensityAugment.apply: intensity row {j}: seed {seed!r} (an integer in 0 .. 2^32 - 1)")
        for k, name in ((_NSIGMA, "noise sigma"), (_BSIGMA, "blur sigma"), (_F, "contrast factor"), (_G, "gamma")):
            if not np.isfinite(row[k]) or not row[k] > 0:
                raise ValueError(f"IntensityAugment.apply: intensity row {j}: {name} {row[k]!r} must be finite and positive")
        if not np.isfinite(row[_NCLIP]) or row[_NCLIP] < 0:
            raise ValueError(f"IntensityAugment.apply: intensity row {j}: noise clip {row[_NCLIP]!r} must be finite and non-negative")
        for z in row[_Z0:]:
            if not np.isfinite(z) or not 0.0 < z <= 1.0:
                raise ValueError(f"IntensityAugment.apply: intensity row {j}: low-resolution zoom {z!r} must be finite and in (0, 1]")
        rows.append(tuple(row))
    return rows


class IntensityAugment:
    """The intensity stage for patches of ``roi``.  ``apply(image, params=None)`` transforms ``image`` ``[B,1,*roi]`` (or ``[B,*roi]``)
    fp32 IN PLACE with the rows ``params`` (``draw(B)`` when not given) and returns it; batches of more than 16 go as chunks of 16.
    The keyword arguments are those of ``draw_intensity_params``; every one is checked here, and so is the blur's reach: the largest
    radius ``int(4 * sigma + 0.5)`` must not exceed 12 nor the smallest extent of ``roi`` (one reflection must suffice), and
    ``roi[2] <= 4096`` when the blur is on.  The object owns the scratch buffer of blur and low resolution (16 patches, allocated at
    the first batch that needs it and kept), the statistics' workspace, and ``stats``: after an ``apply`` in which some sample drew a
    transform, a device tensor ``[B,4]`` fp32 whose row ``b`` holds ``(min, max, mean, 0)`` of sample ``b`` as contrast and gamma saw it
    (after noise, blur and low resolution); rows of samples that drew neither are 0.  With ``lowres_prob > 0`` the rows of ``draw``
    have 15 values, otherwise 11; ``apply`` takes both.  ``enabled`` is False when every probability is 0: ``draw`` then draws nothing,
    and an ``apply`` whose rows are all off launches nothing and leaves ``stats`` as it was.

    Multi-modal batches: ``apply`` also takes ``[B,C,*roi]``.  The kernels treat a batch as independent patches of ``roi``, so it is
    ``B * C`` of them, sample-major and channel-minor, in chunks of 16 as ever, and ``stats`` is ``[B * C, 4]``.  ``per_channel=True``
    (the default; nnU-Net's ``per_channel``): ``draw(B, channels=C)`` returns ``B * C`` rows, each drawn exactly as a row is drawn for a
    single-channel sample, in that order, and contrast, gamma and their min / max / mean are per channel.  ``per_channel=False``: ``B``
    rows, each used for the ``C`` channels of its sample (the statistics are still per channel), except that channel ``c`` takes the
    noise seed ``(seed + c) mod 2^32``, so that the channels do not receive the same noise field.  With ``C = 1`` both settings draw and
    compute exactly what a single-channel batch always did."""

    def __init__(self, roi: Sequence[int] = (96, 96, 96), rng=np.random, per_channel: bool = True, **keywords):
        self.per_channel = bool(per_channel)
        self.roi = tuple(int(v) for v in roi)
        if len(self.roi) != 3 or min(self.roi) < 1 or self.roi[0] * self.roi[1] * self.roi[2] > 2 ** 31 - 1:
            raise ValueError(f"IntensityAugment: roi {tuple(roi)}: three positive extents of at most 2^31 - 1 voxels expected")
        self.rng = rng
        self._args = _intensity_arguments(**keywords)
        self.keywords = keywords
        blur_prob, blur_sigma = self._args[3], self._args[4]
        if blur_prob > 0:
            r = blur_radius(blur_sigma[-1])
            if r > min(self.roi):
                raise ValueError(f"IntensityAugment: blur_sigma {blur_sigma}: the radius {r} exceeds the smallest extent of roi {self.roi}")
            if self.roi[2] > BLUR_MAX_LINE:
                raise ValueError(f"IntensityAugment: roi {self.roi}: the blur takes at most {BLUR_MAX_LINE} voxels along the last axis")
        self.enabled = any(self._args[k] > 0 for k in (0, 3, 5, 7, 10))
        self.stats: Optional[torch.Tensor] = None
        self._scratch: Optional[torch.Tensor] = None
        self._ws: Optional[torch.Tensor] = None

    def draw(self, n: int, channels: int = 1) -> List[tuple]:
        """The rows of ``n`` samples of ``channels`` channels: with ``per_channel`` ``n * channels`` rows, sample-major and
        channel-minor, each drawn exactly as a single row is (so they are ``n * channels`` consecutive draws); without it ``n`` rows."""
        return [_draw_row(self.rng, *self._args) for _ in range(int(n) * (int(channels) if self.per_channel else 1))]

    def _patch_rows(self, params, n: int, channels: int) -> List[tuple]:
        """One checked row per patch of a ``[n, channels, *roi]`` batch, sample-major and channel-minor.  ``per_channel``: ``params``
        are those rows.  Otherwise ``params`` are ``n`` rows and channel ``c`` of a sample takes the sample's row with the noise seed
        ``(seed + c) mod 2^32``: one decision and one factor for the sample, but no two channels receive the same noise field."""
        want = n * channels if self.per_channel else n
        if channels > 1 and len(params) != want:
            what = f"per sample and channel ({n} x {channels})" if self.per_channel else f"per sample ({n}; per_channel is off)"
            raise ValueError(f"IntensityAugment.apply: a contiguous fp32 batch [{n},{channels},*roi] takes one intensity row of "
                             f"{ROW_LENGTH} values {what}, got {len(params)}")
        if self.per_channel or channels == 1:
            return _checked_rows(params, n * channels)
        rows = []
        for row in _checked_rows(params, n):
            for c in range(channels):
                rows.append(row[:_SEED] + ((int(row[_SEED]) + c) % 2 ** 32,) + row[_SEED + 1:])
        return rows

    def _buffer(self, name: str, numel: int, dtype, dev) -> torch.Tensor:
        t = getattr(self, name)
        if t is None or t.device != dev:
            t = torch.empty(numel, dtype=dtype, device=dev)
            setattr(self, name, t)
        return t

    def apply(self, image: torch.Tensor, params: Optional[Sequence[Sequence[float]]] = None) -> torch.Tensor:
        roi = self.roi
        if not torch.is_tensor(image) or image.dtype != torch.float32 or not image.is_contiguous() or image.ndim not in (4, 5) \
                or tuple(image.shape[-3:]) != roi or (image.ndim == 5 and image.shape[1] < 1) or image.shape[0] < 1:
            got = f"{tuple(image.shape)} {image.dtype}, contiguous {image.is_contiguous()}" if torch.is_tensor(image) else type(image).__name__
            raise ValueError(f"IntensityAugment.apply: a contiguous fp32 tensor [B,C,{roi[0]},{roi[1]},{roi[2]}] expected, got {got}")
        dev = image.device
        if dev.type != "cuda" and not _lib.host_pointers_ok():
            raise ValueError(f"IntensityAugment.apply: the batch must be on a HIP device, got {dev}")
        channels = int(image.shape[1]) if image.ndim == 5 else 1
        samples = int(image.shape[0])
        rows = self._patch_rows(self.draw(samples, channels) if params is None else params, samples, channels)
        n = samples * channels                           # the kernels see n independent patches of roi, sample-major and channel-minor
        # the low extents per sample; roi itself where the sample did not draw low resolution (and where every zoom rounds to it)
        extents = [lowres_extents(roi, r[_Z0:]) if len(r) == LOWRES_ROW_LENGTH and r[_LOWRES] else roi for r in rows]
        if not any(r[k] for r in rows for k in (_NOISE, _BLUR, _CONTRAST, _GAMMA)) and all(e == roi for e in extents):
            return image                                 # nothing drawn: nothing is launched, not even a fill
        need_stats = [int(bool(r[_CONTRAST] or r[_GAMMA])) for r in rows]
        self.stats = torch.zeros((n, 4), dtype=torch.float32, device=dev)
        per = roi[0] * roi[1] * roi[2]
        flat = image.view(n, per)
        L = _lib.lib()
        stream = _lib.stream_of(dev)
        for lo in range(0, n, INTENSITY_MAX_BATCH):
            chunk = rows[lo:lo + INTENSITY_MAX_BATCH]
            m = len(chunk)
            ptr = flat[lo:].data_ptr()
            if any(r[_NOISE] for r in chunk):
                p = (ctypes.c_double * (4 * m))(*[float(v) for r in chunk for v in (r[_NOISE], r[_SEED], r[_NSIGMA], r[_NCLIP])])
                _lib.check(L.icl_intensity_noise(ptr, p, m, *roi, stream), "intensity_noise")
            if any(r[_BLUR] and blur_radius(r[_BSIGMA]) > 0 for r in chunk):
                scratch = self._buffer("_scratch", INTENSITY_MAX_BATCH * per, torch.float32, dev)
                vals = []
                for r in chunk:
                    w = blur_weights(r[_BSIGMA]) if r[_BLUR] and blur_radius(r[_BSIGMA]) <= BLUR_MAX_RADIUS else np.ones(1)
                    vals += [float(r[_BLUR]), float(r[_BSIGMA]), *w, *([0.0] * (BLUR_MAX_RADIUS + 1 - len(w)))]
                p = (ctypes.c_double * len(vals))(*vals)
                _lib.check(L.icl_intensity_blur(ptr, scratch.data_ptr(), p, m, *roi, stream), "intensity_blur")
            low = extents[lo:lo + m]
            if any(e != roi for e in low):
                scratch = self._buffer("_scratch", INTENSITY_MAX_BATCH * per, torch.float32, dev)
                p = (ctypes.c_int32 * (4 * m))(*[v for e in low for v in (int(e != roi), *e)])
                _lib.check(L.icl_intensity_lowres(ptr, scratch.data_ptr(), p, m, *roi, stream), "intensity_lowres")
            if any(need_stats[lo:lo + m]):
                ws = self._buffer("_ws", INTENSITY_WS_DOUBLES, torch.float64, dev)
                flags = (ctypes.c_int32 * m)(*need_stats[lo:lo + m])
                stats = self.stats[lo:].data_ptr()
                _lib.check(L.icl_intensity_stats(ptr, flags, m, *roi, stats, ws.data_ptr(), stream), "intensity_stats")
                p = (ctypes.c_double * (5 * m))(*[float(v) for r in chunk for v in (r[_CONTRAST], r[_F], r[_GAMMA], r[_G], r[_INVERT])])
                _lib.check(L.icl_intensity_point(ptr, stats, p, m, *roi, stream), "intensity_point")
        return image


def _intensity_rows(intensity: Optional[IntensityAugment], roi: Sequence[int], n: int, intensity_params, who: str, channels: int = 1):
    """What the loaders share: the intensity rows of a batch of ``n`` samples of ``channels`` channels, drawn here (after the batch's
    geometric rows) when the caller gave none; None without a stage."""
    if intensity is None:
        if intensity_params is not None:
            raise ValueError(f"{who}: intensity_params given, but the loader has no intensity stage")
        return None
    if tuple(intensity.roi) != tuple(roi):
        raise ValueError(f"{who}: the intensity stage is for patches of {intensity.roi}, the loader's are {tuple(roi)}")
    return intensity.draw(n, channels) if intensity_params is None else intensity_params


def _check_stage(intensity, roi: Sequence[int], who: str):
    if intensity is not None and (not isinstance(intensity, IntensityAugment) or tuple(intensity.roi) != tuple(int(v) for v in roi)):
        raise ValueError(f"{who}: intensity must be an IntensityAugment for patches of {tuple(roi)}")
