"""Data feed of the 3-D AMOS trainer on the device (``train_inherent_consistent_unet_3D_AMOS22.py``).

What the reference does (``:84-138,182-197``): MONAI dictionary transforms in a ``CacheDataset`` behind a ``ThreadDataLoader``.
The deterministic prefix (``LoadImaged … Spacingd``, ``:86-101``) is computed once and cached; the random tail (``:102-133``) runs on
host threads for every sample of every batch:

    RandSpatialCropd(roi 96^3, random_size=False) -> SpatialPadd(96^3) -> RandFlipd(axis 0) -> RandFlipd(axis 1) -> RandFlipd(axis 2)
    -> RandRotate90d(max_k=3) -> RandShiftIntensityd(offsets 0.10)

Here the cached volumes stay resident in HBM (``DeviceVolumeStore``, filled by ``amos_volume_store``), the host draws the random
parameters of a batch (``draw_amos_params``) and ONE gather kernel (``volume_feed_kernel`` in ``csrc/kernels/datafeed.h``, through
``icl_volume_feed``) produces the batch.  ``AMOSDeviceLoader`` stands where the ``ThreadDataLoader`` stood.

**The cached prefix** (``ScaleIntensityRanged -> CropForegroundd -> Orientationd("RAS") -> Spacingd``, ``:86-101``; validation, ``:141-154``,
with ``SpatialPadd(96^3)`` before ``Spacingd``) runs on the device too, from the raw arrays and the affine the caller read from the file
(no NIfTI is read here).  ``plan_prefix`` describes a case as a value on the host (``PrefixPlan``: foreground box, permutation and signs
from ``orientation_from_affine`` — nibabel's ``io_orientation`` restated —, spacings, pad, extents); ``amos_prefix`` finds the box
(``icl_prefix_box``; its six integers are the only read-back), then windows, crops, reorients, pads and respaces image and label in ONE
gather from the raw arrays (``icl_prefix_resample``, ``csrc/kernels/prefix.h``); ``amos_volume_store_from_raw`` fills the store that way
and ``amos_val_cases_from_raw`` makes the validation items; ``restore_label`` is the inverse for label maps (MONAI's ``Invertd`` on a
prediction).  The definition is in DESIGN.md §2 "AMOS cached prefix"; ``tests/amos_prefix_ref.py`` restates it as the literal numpy
chain, which the emulated kernels and the GPU equal bit for bit.  Parity with MONAI's own code is unpinned here as well.

**Parity with MONAI's own code is unpinned.**  MONAI is not installed where this package is built and tested, so the transform
semantics are restated from MONAI 1.0.1's published definitions (as the window grid and the Gaussian map of ``val_3D`` are) and no golden
vector of MONAI's output exists.  What the tests pin is the kernel against a numpy restatement of the forward chain
(``tests/amos_feed_ref.py``) and the order and number of the random draws documented at ``draw_amos_params``.  MONAI gives every
transform a generator of its own; here one generator serves all of them, so the batches are distributed like MONAI's, not equal to them.

**Random rotation and zoom** (MONAI ``RandAffined``, nnU-Net's rotation and scaling; off by default: ``affine_prob=0``).  Both feeds
take an affine stage between the pad and the flips: the host draws three angles and one or three zooms, ``affine_matrix`` forms the 3x3
``M`` in double, and ``volume_feed_affine_kernel`` (``icl_volume_feed_affine`` / ``icl_volume_feed_affine_origins``) interpolates the
image trilinearly and takes the label's nearest voxel, about the patch centre, from the WHOLE volume (zeros only outside it).  The
definition is in DESIGN.md §2 "Affine stage of the 3-D feed"; ``tests/affine_feed_ref.py`` restates it in numpy, which the emulated
kernel and the GPU equal bit for bit.  MONAI's ``RandAffine`` samples the cropped patch, this gather samples the volume: unpinned too.

**Foreground-balanced crops** (``utils/data_utils.py:84-99``, ``get_loader``: ``RandCropByPosNegLabeld(pos=1, neg=1, num_samples=4,
image_threshold=0)``, the crop of every MONAI recipe for AMOS or BTCV).  MONAI keeps two int64 index lists per cached volume on the host.
Here ``ForegroundIndex`` builds a rank index per volume on the device (``csrc/kernels/rankindex.h``: one prefix count per 1,024 voxels
and list, under 1 % of the volume) and reads back the two list lengths once; ``draw_posneg_params`` draws "the r-th foreground voxel" on
the host in MONAI's order; ``OnDeviceAugmentPosNeg.batch`` turns the ranks into crop origins with one select launch and gathers with
``icl_volume_feed_origins``, which reads the origins from device memory: no step synchronises with the host.  Parity with MONAI's own
code is unpinned here too; what ``tests/posneg_feed_ref.py`` pins is the algorithm documented at ``draw_posneg_params``.
"""
from __future__ import annotations

import ctypes
import dataclasses
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _lib
from .affine import (AFFINE_MAX_ENTRY, _affine_arguments, _affine_block, _affine_suffixes, _draw_affine,      # noqa: F401  (re-exported)
                     affine_matrix)
from .brats2019 import FEED_MAX_BATCH, DeviceVolumeStore      # noqa: F401  (FEED_MAX_BATCH is re-exported)
from .intensity import _check_stage, _intensity_rows


def draw_amos_params(shape: Sequence[int], roi: Sequence[int], rng=np.random, flip_prob: float = 0.10, rot_prob: float = 0.10,
                     max_k: int = 3, shift_offset: float = 0.10, shift_prob: float = 0.50, scale_factor: float = 0.0,
                     scale_prob: float = 0.0, affine_prob: float = 0.0, rotate_range=(0, 0, 0), zoom_range=(1.0, 1.0),
                     zoom_isotropic: bool = True) -> tuple:
    """The random draws of the AMOS trainer's transforms (``:102-133``) for one volume of ``shape``, from ``rng`` (``np.random`` or a
    ``RandomState``), in this fixed order:

    1. crop (``RandSpatialCrop``, ``random_size=False``): the size is ``s = min(roi, n)`` per axis; per axis, in order,
       ``origin = rng.randint(0, n - s + 1)`` ONLY IF ``n > s``, otherwise the origin is 0 and nothing is drawn;
    2. pad (``SpatialPad``, symmetric): ``w = roi - s``, ``w // 2`` on the left, the rest on the right; nothing is drawn;
    2a. affine (rotation and zoom about the patch centre, off by default): with ``affine_prob == 0`` nothing is drawn at all; otherwise
       ``rng.rand() < affine_prob`` and, only if true, ``theta_a = rng.uniform(-r_a, r_a)`` for a = 0, 1, 2 (always three draws;
       ``rotate_range`` in radians, one number meaning all three axes), then ONE ``z = rng.uniform(lo, hi)`` of ``zoom_range`` when
       ``zoom_isotropic``, or three when not; the sample's matrix is ``affine_matrix(theta, z)``;
    3. flips: for axis 0, 1, 2 in turn, ``rng.rand() < flip_prob``;
    4. rotation: ``rng.rand() < rot_prob``; ONLY IF true, ``k = rng.randint(max_k) + 1`` (otherwise ``k = 0``);
    5. scale (``RandScaleIntensity``; off by default — the AMOS trainer has none, ``utils/data_utils.py:98`` has one): with
       ``scale_prob == 0`` nothing is drawn at all; otherwise ``rng.rand() < scale_prob`` and, only if true,
       ``mul = float32(1 + rng.uniform(-scale_factor, scale_factor))``;
    6. shift (``RandShiftIntensity``): ``rng.rand() < shift_prob``; ONLY IF true, ``add = float32(rng.uniform(-o, o))``.

    Returns one ``icl_volume_feed`` parameter row: 14 integers ``(n0, n1, n2, c0, c1, c2, s0, s1, s2, l0, l1, l2, flip mask, k)``
    followed by the two floats ``(mul, add)``: 16 values.  A sample that drew an affine carries the nine entries of ``M``, row-major,
    behind them: 25 values."""
    affine = _affine_arguments(affine_prob, rotate_range, zoom_range, zoom_isotropic)
    n = [int(v) for v in shape]
    r = [int(v) for v in roi]
    if len(n) != 3 or len(r) != 3 or min(n) < 1 or min(r) < 1:
        raise ValueError(f"draw_amos_params: shape {tuple(shape)} and roi {tuple(roi)} must be three positive extents each")
    size = [min(r[a], n[a]) for a in range(3)]
    origin = [int(rng.randint(0, n[a] - size[a] + 1)) if n[a] > size[a] else 0 for a in range(3)]
    left = [(r[a] - size[a]) // 2 for a in range(3)]
    matrix = _draw_affine(rng, *affine)
    return (*n, *origin, *size, *left, *_draw_tail(rng, flip_prob, rot_prob, max_k, shift_offset, shift_prob, scale_factor, scale_prob), *matrix)


def _draw_tail(rng, flip_prob, rot_prob, max_k, shift_offset, shift_prob, scale_factor, scale_prob) -> tuple:
    """Steps 3-6 of ``draw_amos_params``: ``(flip mask, k, mul, add)``."""
    flip = 0
    for a in range(3):
        if rng.rand() < flip_prob:
            flip |= 1 << a
    k = 0
    if rng.rand() < rot_prob:
        k = int(rng.randint(max_k)) + 1
    mul, add = np.float32(1.0), np.float32(0.0)
    if scale_prob > 0 and rng.rand() < scale_prob:
        mul = np.float32(1 + rng.uniform(-scale_factor, scale_factor))
    if rng.rand() < shift_prob:
        add = np.float32(rng.uniform(-shift_offset, shift_offset))
    return flip, k, float(mul), float(add)


def _as_label_u8(label: np.ndarray) -> np.ndarray:
    """Float or integer label values -> uint8; fractional, non-finite or out-of-range values are an error."""
    label = np.asarray(label)
    if label.dtype == np.uint8:
        return label
    if label.dtype.kind == "f":
        if not np.isfinite(label).all() or (label != np.floor(label)).any():
            raise ValueError("amos_volume_store: a label map holds fractional or non-finite values")
    elif label.dtype.kind not in "iub":
        raise ValueError(f"amos_volume_store: label dtype {label.dtype}")
    if label.size and (label.min() < 0 or label.max() > 255):
        raise ValueError("amos_volume_store: label values outside 0..255")
    return label.astype(np.uint8)


def _host_array(x) -> np.ndarray:
    if torch.is_tensor(x):                       # MONAI's MetaTensor is a torch.Tensor subclass
        x = x.detach().cpu().numpy()
    return np.asarray(x)


def amos_volume_store(samples: Iterable, device) -> DeviceVolumeStore:
    """A ``DeviceVolumeStore`` from what ``CacheDataset`` caches for the AMOS trainer: an iterable of ``{'image': …, 'label': …}``
    dictionaries (or ``(image, label)`` pairs) whose arrays are channel-first ``[1, W, H, D]`` (``ensure_channel_first=True``; plain
    ``[W, H, D]`` is taken too), the label float32 with integer values (``LoadImaged`` yields float32).  The image goes up as fp32, the
    label as uint8; a label with fractional, non-finite or out-of-range (outside 0..255) values raises ``ValueError``."""
    volumes = []
    for sample in samples:
        image, label = (sample["image"], sample["label"]) if isinstance(sample, dict) else sample
        image, label = _host_array(image), _host_array(label)
        if image.ndim == 4 and label.ndim == 4:
            if image.shape[0] != 1 or label.shape[0] != 1:
                raise ValueError(f"amos_volume_store: one channel expected, got image {image.shape} and label {label.shape}")
            image, label = image[0], label[0]
        if image.ndim != 3 or image.shape != label.shape:
            raise ValueError(f"amos_volume_store: image {image.shape} and label {label.shape} must be [1,W,H,D] (or [W,H,D]) of one extent")
        volumes.append((image, _as_label_u8(label)))
    return DeviceVolumeStore(volumes, device)


def _single_channel_store(store, who: str):
    """The AMOS feeds, the rank index and the cached prefix take ``[W,H,D]`` volumes only."""
    if getattr(store, "multichannel", False):
        raise ValueError(f"{who}: the store holds multi-channel [{store.channels},W,H,D] volumes; the AMOS feeds are single-channel "
                         "(CT is one channel): use dataloaders.brats2019.OnDeviceAugment for multi-modal volumes")


class OnDeviceAugmentAMOS:
    """The random transforms of the AMOS trainer (``:102-133``) + batch collation on the GPU.  ``batch(indices)`` returns
    ``{'image': [B,1,*roi] fp32, 'label': [B,1,*roi] int64}``: the label carries MONAI's channel axis, so the trainer's
    ``label_batch[:labeled_bs].squeeze(1).long()`` and ``.long()`` (``:225-227``) work unchanged.  Difference to the reference: its
    loader yields a FLOAT32 label there (``ToTensord`` is given the image only and ``LoadImaged`` loads float32); here it is int64
    already and the ``.long()`` calls are no-ops.

    The keyword arguments are those of ``draw_amos_params`` (``flip_prob``, ``rot_prob``, ``max_k``, ``shift_offset``, ``shift_prob``,
    ``scale_factor``, ``scale_prob``, and the affine stage's ``affine_prob``, ``rotate_range``, ``zoom_range``, ``zoom_isotropic``, which
    are checked here) plus ``rng`` (default: numpy's global generator).  With ``affine_prob=0`` (the default) nothing is drawn for
    the stage and ``batch`` launches what it launched before the stage existed.

    ``intensity``: None, or an ``IntensityAugment`` for the same ``roi`` (``dataloaders/intensity.py``: Gaussian noise, blur, contrast
    and gamma).  ``batch`` then draws the batch's intensity rows AFTER all of its geometric rows, in sample order, from the stage's own
    ``rng`` (pass the loader's generator to the stage to keep one stream), and applies the stage in place behind the gather, on the
    same stream.  With None, or a stage whose probabilities are all 0, nothing is drawn or launched for it.

    Single-channel only (CT is one channel): a store of ``[C,W,H,D]`` volumes is refused with a ``ValueError``, by this feed, its
    affine stage and ``OnDeviceAugmentPosNeg`` alike; multi-modal volumes go through ``dataloaders.brats2019.OnDeviceAugment``."""

    def __init__(self, store: DeviceVolumeStore, roi: Sequence[int] = (96, 96, 96), rng=np.random, intensity=None, **probabilities):
        _single_channel_store(store, type(self).__name__)
        self.store = store
        self.roi = tuple(int(v) for v in roi)
        if len(self.roi) != 3 or min(self.roi) < 1:
            raise ValueError(f"OnDeviceAugmentAMOS: roi {tuple(roi)}")
        self.rng = rng
        _check_stage(intensity, self.roi, type(self).__name__)
        self.intensity = intensity
        draw_amos_params((1, 1, 1), self.roi, np.random.RandomState(0), **probabilities)      # rejects unknown keywords here, not mid-epoch
        self.probabilities = probabilities
        if self.roi[0] != self.roi[1] and probabilities.get("rot_prob", 0.10) > 0 and probabilities.get("max_k", 3) >= 1:
            raise ValueError(f"OnDeviceAugmentAMOS: roi {self.roi} is not square in axes (0, 1), so a quarter turn would change the "
                             "patch's shape (MONAI's loader could not collate such a batch either): pass rot_prob=0")

    def draw(self, indices: Sequence[int]) -> List[tuple]:
        return [draw_amos_params(self.store.images[i].shape, self.roi, self.rng, **self.probabilities) for i in indices]

    def _outputs(self, n: int, out) -> Tuple[torch.Tensor, torch.Tensor]:
        dev = self.store.device
        if out is None:
            return (torch.empty((n, 1) + self.roi, dtype=torch.float32, device=dev),
                    torch.empty((n, 1) + self.roi, dtype=torch.int64, device=dev))
        image, label = out
        for name, t, dtype, shapes in (("image", image, torch.float32, [(n, 1) + self.roi]),
                                       ("label", label, torch.int64, [(n, 1) + self.roi, (n,) + self.roi])):
            same_device = torch.is_tensor(t) and t.device.type == dev.type and (dev.index is None or t.device.index == dev.index)
            if not same_device or t.dtype != dtype or tuple(t.shape) not in shapes or not t.is_contiguous():
                got = f"{tuple(t.shape)} {t.dtype} on {t.device}, contiguous {t.is_contiguous()}" if torch.is_tensor(t) else type(t).__name__
                raise ValueError(f"{type(self).__name__}.batch: out {name} must be a contiguous {dtype} tensor of shape "
                                 f"{' or '.join(map(str, shapes))} on {dev}, got {got}")
        return image, label

    ROW_VALUES = 16             # the fixed part of a parameter row; nine matrix entries may follow it

    def _row_wording(self) -> str:
        return "one parameter row of 16 values per index"

    def _sample_volumes(self, indices: List[int]) -> List[int]:
        """The volume of every sample of the batch."""
        return indices

    def _check_row(self, who: str, i: int, row) -> None:
        """What a subclass checks of a row of volume ``i`` beyond the extents and the quarter turn."""

    def _launch(self, L, chunk, rows, args, affine, outs, stream):
        """The launches of one chunk of at most ``FEED_MAX_BATCH`` samples: ``chunk`` their volumes, ``rows`` their parameter rows,
        ``args = (images, labels, ints, floats)`` as the gather entries take them, ``affine`` the ``_affine_block`` or None, ``outs``
        the image and label addresses of the chunk's first sample."""
        if affine is None:                       # no sample of the launch has an affine: the launch of a loader without the stage
            _lib.check(L.icl_volume_feed(*args, len(chunk), *outs, *self.roi, stream), "volume_feed")
        else:
            _lib.check(L.icl_volume_feed_affine(*args, affine, len(chunk), *outs, *self.roi, stream), "volume_feed_affine")

    def batch(self, indices: Sequence[int], params: Optional[Sequence[Sequence[float]]] = None, out=None, intensity_params=None):
        """One batch for the volumes ``indices`` of the store.  ``params``: one ``draw_amos_params`` row per index (drawn here when
        not given).  ``intensity_params``: one ``draw_intensity_params`` row per sample for the loader's intensity stage (drawn here,
        after ``params``, when not given).  ``out=(image, label)``: write into the caller's tensors — for example ``ICLTrainer.static_vol`` /
        ``static_lab`` after ``capture()``, so that a captured step needs no extra copy — and return views of them; shape
        (``[B,1,*roi]``; the label may also be ``[B,*roi]``), dtype, device and contiguity are checked.  More than 16 indices are
        handled as chunks of 16.

        ``OnDeviceAugmentPosNeg``: one batch of ``len(indices) * num_samples`` samples.  ``params``: ``num_samples``
        ``draw_posneg_params`` rows per index, volume-major; a rank at or past the length of its list is refused here, since only the
        host knows the lengths.  ``intensity_params``: one row per SAMPLE.  More than 16 samples go as chunks of 16."""
        st, who, base = self.store, f"{type(self).__name__}.batch", self.ROW_VALUES
        indices = [int(i) for i in indices]
        if len(indices) < 1:
            raise ValueError(f"{who}: no indices")
        if params is None:
            params = self.draw(indices)
        sample_of = self._sample_volumes(indices)
        n = len(sample_of)
        if len(params) != n:
            raise ValueError(f"{who}: {self._row_wording()}")
        intensity_params = _intensity_rows(self.intensity, self.roi, n, intensity_params, who)
        suffixes = _affine_suffixes(who, params, base, self._row_wording())
        for i, row in zip(sample_of, params):
            if tuple(int(v) for v in row[:3]) != tuple(st.images[i].shape):
                raise ValueError(f"{who}: parameter row for extents {tuple(row[:3])}, volume {i} is {tuple(st.images[i].shape)}")
            if int(row[13]) & 1 and self.roi[0] != self.roi[1]:
                raise ValueError(f"{who}: k = {int(row[13])} with roi {self.roi}: an odd quarter turn needs roi[0] == roi[1]")
            self._check_row(who, i, row)
        image, label = self._outputs(n, out)
        per = self.roi[0] * self.roi[1] * self.roi[2]
        flat_image, flat_label = image.view(n, per), label.view(n, per)
        L = _lib.lib()
        stream = _lib.stream_of(st.device)
        for lo in range(0, n, FEED_MAX_BATCH):
            chunk, rows = sample_of[lo:lo + FEED_MAX_BATCH], params[lo:lo + FEED_MAX_BATCH]
            m = len(chunk)
            ptrs = ctypes.c_void_p * m
            args = (ptrs(*[st.images[i].data_ptr() for i in chunk]), ptrs(*[st.labels[i].data_ptr() for i in chunk]),
                    (ctypes.c_int32 * (14 * m))(*[int(v) for row in rows for v in row[:14]]),
                    (ctypes.c_float * (2 * m))(*[float(v) for row in rows for v in row[14:16]]))
            self._launch(L, chunk, rows, args, _affine_block(suffixes[lo:lo + m]), (flat_image[lo:].data_ptr(), flat_label[lo:].data_ptr()),
                         stream)
        if intensity_params is not None:
            self.intensity.apply(image, intensity_params)
        return {"image": image, "label": label.view((n, 1) + self.roi)}


KIND_FG, KIND_BG = 0, 1     # the list a centre is drawn from (kRankFg / kRankBg of csrc/kernels/rankindex.h)


def rank_tile() -> int:
    """Consecutive flat voxels per entry of a rank index (``kRankTile``)."""
    return int(_lib.lib().icl_rank_tile())


class ForegroundIndex:
    """The rank indices of every volume of ``store`` for ``RandCropByPosNegLabel``'s two lists, ``fg = label != 0`` and
    ``bg = (image > image_threshold) & (label == 0)`` (a NaN voxel is not above the threshold): ``fg[i]`` / ``bg[i]`` are device
    ``int32`` tensors of ``tiles + 1`` entries holding the uint32 prefix counts of ``csrc/kernels/rankindex.h`` (``tiles =
    ceil(voxels / rank_tile())``; the last entry is the length of the list), ``n_fg[i]`` / ``n_bg[i]`` those lengths on the host.
    Building it is the single read-back of the pos/neg feed: all totals travel in one copy after the last launch.  An extent of
    65,536 or more (MONAI's ``uint16`` centres) or more than 2^31 - 1 voxels is refused, and so is a store of multi-channel
    ``[C,W,H,D]`` volumes (``ValueError``): the index, like the feeds it serves, is single-channel."""

    def __init__(self, store: DeviceVolumeStore, image_threshold: float = 0.0):
        _single_channel_store(store, "ForegroundIndex")
        self.store = store
        self.image_threshold = float(image_threshold)
        self.fg: List[torch.Tensor] = []
        self.bg: List[torch.Tensor] = []
        dev = store.device
        L = _lib.lib()
        tile = rank_tile()
        stream = _lib.stream_of(dev)
        for image, label in zip(store.images, store.labels):
            n = tuple(int(v) for v in image.shape)
            if max(n) > 65535 or n[0] * n[1] * n[2] > 2 ** 31 - 1:
                raise ValueError(f"ForegroundIndex: extents {n}: each must be below 65,536 and the volume at most 2^31 - 1 voxels")
            entries = -(-(n[0] * n[1] * n[2]) // tile) + 1
            fg = torch.empty(entries, dtype=torch.int32, device=dev)
            bg = torch.empty(entries, dtype=torch.int32, device=dev)
            _lib.check(L.icl_rank_index_build(image.data_ptr(), label.data_ptr(), *n, self.image_threshold, fg.data_ptr(), bg.data_ptr(),
                                              stream), "rank_index_build")
            self.fg.append(fg)
            self.bg.append(bg)
        if self.fg:
            totals = torch.stack([t[-1] for pair in zip(self.fg, self.bg) for t in pair]).cpu().numpy().astype(np.int64) & 0xffffffff
        else:
            totals = np.zeros(0, dtype=np.int64)
        self.n_fg = [int(v) for v in totals[0::2]]
        self.n_bg = [int(v) for v in totals[1::2]]

    def __len__(self):
        return len(self.fg)


def draw_posneg_params(shape: Sequence[int], roi: Sequence[int], n_fg: int, n_bg: int, rng=np.random, pos: float = 1, neg: float = 1,
                       num_samples: int = 4, **probabilities) -> List[tuple]:
    """The random draws of ``RandCropByPosNegLabeld(pos, neg, num_samples)`` followed by the tail of ``draw_amos_params`` for one
    volume of ``shape`` whose lists hold ``n_fg`` foreground and ``n_bg`` background voxels (``ForegroundIndex``), from ONE generator:

    1. ``pos_ratio = pos / (pos + neg)``; both lists empty: ``ValueError("No sampling location available")``; exactly one list empty:
       ``pos_ratio`` becomes 0 (no foreground) or 1 (no background), and the draws below are still made;
    2. centres, for each of the ``num_samples`` crops in order: ``use_fg = rng.rand() < pos_ratio``, then
       ``rank = rng.randint(len(list))`` of the chosen list: the centre is ``unravel_index(list[rank], shape)``;
    3. then, for crop 0, 1, ..., the affine draw (step 2a of ``draw_amos_params``; nothing with ``affine_prob == 0``) followed by the
       tail draws, steps 3-6 of ``draw_amos_params`` (flips, rotation, scale, shift).

    The crop has the size ``s = min(roi, n)`` and the origin ``clamp(centre - s // 2, 0, n - s)`` per axis (``correct_crop_centers``
    followed by ``SpatialCrop(roi_center, roi_size)``); the device computes it from the rank, so the origin fields of a row are unused
    (0).  Returns ``num_samples`` rows: the 16 values of a ``draw_amos_params`` row followed by ``(kind, rank)``, ``kind`` being
    ``KIND_FG`` (0) or ``KIND_BG`` (1): 18 values, and behind them the nine entries of ``M`` for a crop that drew an affine (27).  The
    keyword arguments are the probabilities of ``draw_amos_params``, its four affine keywords included."""
    n = [int(v) for v in shape]
    r = [int(v) for v in roi]
    if len(n) != 3 or len(r) != 3 or min(n) < 1 or min(r) < 1:
        raise ValueError(f"draw_posneg_params: shape {tuple(shape)} and roi {tuple(roi)} must be three positive extents each")
    if pos < 0 or neg < 0 or pos + neg == 0:
        raise ValueError(f"draw_posneg_params: pos = {pos} and neg = {neg} must be non-negative and not both 0")
    num_samples, n_fg, n_bg = int(num_samples), int(n_fg), int(n_bg)
    if num_samples < 1 or n_fg < 0 or n_bg < 0:
        raise ValueError(f"draw_posneg_params: num_samples {num_samples}, n_fg {n_fg}, n_bg {n_bg}")
    probabilities = dict(probabilities)
    affine = _affine_arguments(**{key: probabilities.pop(key) for key in _AFFINE_KEYWORDS if key in probabilities})
    tail = _tail_arguments(**probabilities)
    pos_ratio = pos / (pos + neg)
    if n_fg == 0 or n_bg == 0:
        if n_fg == 0 and n_bg == 0:
            raise ValueError("No sampling location available")
        pos_ratio = 0 if n_fg == 0 else 1
    centres = []
    for _ in range(num_samples):
        kind = KIND_FG if rng.rand() < pos_ratio else KIND_BG
        centres.append((kind, int(rng.randint(n_fg if kind == KIND_FG else n_bg))))
    size = [min(r[a], n[a]) for a in range(3)]
    left = [(r[a] - size[a]) // 2 for a in range(3)]
    rows = []
    for kind, rank in centres:
        matrix = _draw_affine(rng, *affine)                      # drawn before the crop's flips, as in draw_amos_params
        rows.append((*n, 0, 0, 0, *size, *left, *_draw_tail(rng, *tail), kind, rank, *matrix))
    return rows


_AFFINE_KEYWORDS = ("affine_prob", "rotate_range", "zoom_range", "zoom_isotropic")


def _tail_arguments(flip_prob: float = 0.10, rot_prob: float = 0.10, max_k: int = 3, shift_offset: float = 0.10, shift_prob: float = 0.50,
                    scale_factor: float = 0.0, scale_prob: float = 0.0) -> tuple:
    """``draw_amos_params``' probabilities with its defaults, in ``_draw_tail``'s order; an unknown keyword is a ``TypeError``."""
    return flip_prob, rot_prob, max_k, shift_offset, shift_prob, scale_factor, scale_prob


class OnDeviceAugmentPosNeg(OnDeviceAugmentAMOS):
    """``RandCropByPosNegLabeld(pos, neg, num_samples, image_threshold)`` -> ``SpatialPadd`` -> the AMOS tail (three flips, ``rot90``,
    scale, shift) + batch collation on the GPU: the train loader of ``utils/data_utils.py`` ``get_loader``.  ``batch(indices)`` of
    ``B`` volume indices returns ``{'image': [B*num_samples,1,*roi] fp32, 'label': [B*num_samples,1,*roi] int64}``, volume-major (the
    ``num_samples`` crops of the first volume, then those of the second, ...), which is what MONAI's collate of the per-volume lists
    gives.  ``index``: the ``ForegroundIndex`` of ``store`` (its threshold is ``image_threshold``).  Per chunk of 16 samples two
    launches go to the current stream, ``icl_rank_select`` then ``icl_volume_feed_origins``; nothing is read back.  Otherwise the
    contract of ``OnDeviceAugmentAMOS``: the same ``out=`` checks, the same refusal of a ROI that is not square in axes (0, 1), the
    same keyword arguments."""

    def __init__(self, store: DeviceVolumeStore, index: ForegroundIndex, roi: Sequence[int] = (96, 96, 96), pos: float = 1, neg: float = 1,
                 num_samples: int = 4, rng=np.random, intensity=None, **probabilities):
        super().__init__(store, roi, rng, intensity, **probabilities)
        if index.store is not store or len(index) != len(store):
            raise ValueError("OnDeviceAugmentPosNeg: the ForegroundIndex was not built from this store")
        self.index = index
        self.pos, self.neg, self.num_samples = pos, neg, int(num_samples)
        draw_posneg_params((1, 1, 1), self.roi, 1, 1, np.random.RandomState(0), pos, neg, self.num_samples, **probabilities)

    def draw(self, indices: Sequence[int]) -> List[tuple]:
        ix = self.index
        return [row for i in indices for row in draw_posneg_params(self.store.images[i].shape, self.roi, ix.n_fg[i], ix.n_bg[i], self.rng,
                                                                   self.pos, self.neg, self.num_samples, **self.probabilities)]

    ROW_VALUES = 18             # a draw_amos_params row, then (kind, rank)

    def _row_wording(self) -> str:
        return f"{self.num_samples} parameter rows of 18 values per index"

    def _sample_volumes(self, indices: List[int]) -> List[int]:
        return [i for i in indices for _ in range(self.num_samples)]

    def _check_row(self, who: str, i: int, row) -> None:
        kind, rank = int(row[16]), int(row[17])
        if kind not in (KIND_FG, KIND_BG):
            raise ValueError(f"{who}: kind {kind} (0 foreground, 1 background)")
        total = self.index.n_fg[i] if kind == KIND_FG else self.index.n_bg[i]
        if not 0 <= rank < total:
            raise ValueError(f"{who}: rank {rank} outside the {'foreground' if kind == KIND_FG else 'background'} "
                             f"list of volume {i} ({total} voxels)")

    def _launch(self, L, chunk, rows, args, affine, outs, stream):
        ix, m = self.index, len(chunk)
        ptrs = ctypes.c_void_p * m
        origins = torch.empty((m, 3), dtype=torch.int32, device=self.store.device)
        select = (ctypes.c_int32 * (8 * m))(*[int(v) for row in rows for v in (*row[:3], row[16], row[17], *row[6:9])])
        _lib.check(L.icl_rank_select(args[0], args[1], ptrs(*[ix.fg[i].data_ptr() for i in chunk]), ptrs(*[ix.bg[i].data_ptr() for i in chunk]),
                                     select, ix.image_threshold, m, origins.data_ptr(), stream), "rank_select")
        if affine is None:
            _lib.check(L.icl_volume_feed_origins(*args, m, origins.data_ptr(), *outs, *self.roi, stream), "volume_feed_origins")
        else:
            _lib.check(L.icl_volume_feed_affine_origins(*args, affine, m, origins.data_ptr(), *outs, *self.roi, stream),
                       "volume_feed_affine_origins")


class AMOSDeviceLoader:
    """Stands where the AMOS trainer's ``ThreadDataLoader(train_ds, batch_sampler=batch_sampler, …)`` stood (``:196-197``): an
    iterable with ``__len__`` that yields ``augment.batch(indices)`` for the index batches of ``batch_sampler``
    (``TwoStreamBatchSampler``), so ``for i_batch, sampled_batch in enumerate(train_loader)`` runs as written and the loop's ``.cuda()``
    calls are no-ops.  ``augment`` may be an ``OnDeviceAugmentPosNeg``: a batch then holds ``num_samples`` crops per index.  An
    intensity stage travels with ``augment`` (its ``intensity=``): every batch of the loader passes through it."""

    def __init__(self, augment: OnDeviceAugmentAMOS, batch_sampler):
        self.augment = augment
        self.batch_sampler = batch_sampler

    def __len__(self):
        return len(self.batch_sampler)

    def __iter__(self):
        for indices in self.batch_sampler:
            yield self.augment.batch(list(indices))


# ---- the cached prefix: ScaleIntensityRanged -> CropForegroundd -> Orientationd("RAS") -> [SpatialPadd] -> Spacingd, and back -----------

PREFIX_WINDOW = (-175.0, 250.0, 0.0, 1.0, True)     # a_min, a_max, b_min, b_max, clip (:88-90 of the trainer)
PREFIX_PIXDIM = (1.5, 1.5, 2.0)                     # Spacingd(pixdim=…) (:95-99)
PREFIX_BOX_WS_INTS = 6 * 1024                       # int32 words of scratch icl_prefix_box takes (6 * kPrefixBoxBlocks)
_AXCODE = {"R": (0, 1), "L": (0, -1), "A": (1, 1), "P": (1, -1), "S": (2, 1), "I": (2, -1)}


def orientation_from_affine(affine) -> Tuple[Tuple[int, int, int], Tuple[int, int, int], Tuple[float, float, float]]:
    """nibabel's ``io_orientation`` restated, for a 4x4 (or 3x3) affine of a 3-D volume: ``(perm, sign, zooms)`` where RAS-oriented
    axis ``a`` is source axis ``perm[a]``, reversed when ``sign[a]`` is -1, and ``zooms[k]`` is the voxel size of SOURCE axis ``k``.

    ``RZS = A[:3, :3]``; ``zooms = sqrt(sum(RZS ** 2, axis 0))`` (a zero column is a ``ValueError``); ``RS = RZS / zooms``;
    ``P, S, Qt = svd(RS)``; ``tol = S.max() * 3 * eps``; ``R = P[:, keep] @ Qt[keep]`` with ``keep = S > tol``; then for source axis
    0, 1, 2 in turn ``out = argmax |R[:, in]|``, the sign is that of ``R[out, in]``, and row ``out`` of ``R`` is zeroed."""
    A = np.asarray(affine, dtype=np.float64)
    if A.shape not in ((4, 4), (3, 3)) or not np.isfinite(A).all():
        raise ValueError(f"orientation_from_affine: a finite 4x4 (or 3x3) affine expected, got shape {A.shape}")
    RZS = A[:3, :3]
    zooms = np.sqrt(np.sum(RZS * RZS, axis=0))
    if (zooms == 0).any():
        raise ValueError("orientation_from_affine: the affine has a zero column")
    RS = RZS / zooms
    P, S, Qt = np.linalg.svd(RS)
    keep = S > S.max() * 3 * np.finfo(S.dtype).eps
    R = np.dot(P[:, keep], Qt[keep])
    perm, sign = [-1, -1, -1], [0, 0, 0]
    for in_ax in range(3):
        col = R[:, in_ax]
        if np.allclose(col, 0):
            raise ValueError(f"orientation_from_affine: source axis {in_ax} has no direction left (a degenerate affine)")
        out_ax = int(np.argmax(np.abs(col)))
        if perm[out_ax] != -1:
            raise ValueError("orientation_from_affine: two source axes map to one oriented axis")
        perm[out_ax] = in_ax
        sign[out_ax] = -1 if col[out_ax] < 0 else 1
        R[out_ax, :] = 0
    return tuple(perm), tuple(sign), tuple(float(z) for z in zooms)


def orientation_from_axcodes(axcodes) -> Tuple[Tuple[int, int, int], Tuple[int, int, int]]:
    """``(perm, sign)`` as ``orientation_from_affine`` gives them, from three letters naming where source axes 0, 1, 2 point:
    R / A / S positive, L / P / I negative (``"LPS"``: axis 0 runs to the left, axis 1 to the back, axis 2 up)."""
    codes = [str(c).upper() for c in axcodes] if not isinstance(axcodes, str) else list(axcodes.upper())
    if len(codes) != 3 or any(c not in _AXCODE for c in codes):
        raise ValueError(f"orientation_from_axcodes: three letters out of R, L, A, P, S, I expected, got {axcodes!r}")
    perm, sign = [-1, -1, -1], [0, 0, 0]
    for in_ax, c in enumerate(codes):
        out_ax, s = _AXCODE[c]
        if perm[out_ax] != -1:
            raise ValueError(f"orientation_from_axcodes: {axcodes!r} names one anatomical axis twice")
        perm[out_ax], sign[out_ax] = in_ax, s
    return tuple(perm), tuple(sign)


def _window_constants(window) -> Tuple[Tuple[float, float, float, float, float], bool]:
    """``(a_min, a_max, b_min, b_max, clip)`` -> the five fp32 constants of the kernels ``(a_min, a_max - a_min, b_min, b_max - b_min,
    b_max)`` (the differences formed in double, then rounded) and the clip flag."""
    if len(window) != 5:
        raise ValueError(f"plan_prefix: window {window!r}: (a_min, a_max, b_min, b_max, clip) expected")
    a_min, a_max, b_min, b_max = (float(v) for v in window[:4])
    consts = tuple(float(np.float32(v)) for v in (a_min, a_max - a_min, b_min, b_max - b_min, b_max))
    if not all(np.isfinite(consts)) or consts[1] == 0.0:
        raise ValueError(f"plan_prefix: window {window!r}: finite values with a_max != a_min expected")
    return consts, bool(window[4])


@dataclasses.dataclass(frozen=True)
class PrefixPlan:
    """The cached prefix of one case as a value (frozen; made by ``plan_prefix``): ``shape`` raw extents; ``box`` ``(lo0, lo1, lo2, hi0,
    hi1, hi2)`` in raw axes, ``hi`` exclusive; ``perm`` / ``sign``: oriented axis ``a`` is raw axis ``perm[a]`` of the box, reversed when
    ``sign[a]`` is -1; ``spacing`` the source voxel size and ``pixdim`` the target, per ORIENTED axis; ``pad_front`` zeros in front of
    each oriented axis and ``padded_shape`` the extents after ``SpatialPad``; ``out_shape`` the extents after ``Spacing``; ``window`` the
    five fp32 constants ``(a_min, a_max - a_min, b_min, b_max - b_min, b_max)`` and ``clip``."""
    shape: Tuple[int, int, int]
    box: Tuple[int, int, int, int, int, int]
    perm: Tuple[int, int, int]
    sign: Tuple[int, int, int]
    spacing: Tuple[float, float, float]
    pixdim: Tuple[float, float, float]
    pad_front: Tuple[int, int, int]
    padded_shape: Tuple[int, int, int]
    out_shape: Tuple[int, int, int]
    window: Tuple[float, float, float, float, float]
    clip: bool

    @property
    def crop_shape(self) -> Tuple[int, int, int]:
        """Extents of the oriented crop (before the pad)."""
        return tuple(self.box[3 + self.perm[a]] - self.box[self.perm[a]] for a in range(3))

    def int_params(self):
        """The 24 integers ``icl_prefix_resample`` / ``icl_prefix_restore`` take."""
        return (ctypes.c_int32 * 24)(*self.shape, *self.box, *self.perm, *self.sign, *self.pad_front, *self.padded_shape, *self.out_shape)

    def double_params(self):
        return (ctypes.c_double * 6)(*self.spacing, *self.pixdim)

    def window_params(self):
        return (ctypes.c_float * 5)(*self.window)


def prefix_out_extent(extent: int, spacing: float, pixdim: float) -> int:
    """``Spacing``'s output extent of one axis: ``int(rint((extent - 1) * (spacing / pixdim) + 1.0))`` in double, half to even."""
    return int(np.rint(np.float64(extent - 1) * (np.float64(spacing) / np.float64(pixdim)) + 1.0))


def plan_prefix(shape: Sequence[int], box: Sequence[int], affine=None, spacing: Optional[Sequence[float]] = None, axcodes=None,
                pixdim: Sequence[float] = PREFIX_PIXDIM, pad_to: Optional[Sequence[int]] = None, window=PREFIX_WINDOW) -> PrefixPlan:
    """The plan of one case, on the host alone (no device, no library).  ``shape``: raw extents; ``box``: the foreground box ``(lo0, lo1,
    lo2, hi0, hi1, hi2)`` in raw axes, ``hi`` exclusive (``icl_prefix_box`` finds it; an empty one is the ``ValueError`` of a case without
    foreground); the orientation either from ``affine`` (``orientation_from_affine``, which also gives the voxel sizes) or from
    ``spacing=(s0, s1, s2)`` per SOURCE axis together with ``axcodes``; ``pixdim``: the target voxel size per RAS axis; ``pad_to``: None, or
    the extents ``SpatialPad`` grows the oriented crop to before the respacing (validation: ``(96, 96, 96)``), ``w = max(pad_to - extent,
    0)`` zeros per axis of which ``w // 2`` in front; ``window``: ``(a_min, a_max, b_min, b_max, clip)``."""
    n = tuple(int(v) for v in shape)
    if len(n) != 3 or min(n) < 1 or max(n) > 65535 or n[0] * n[1] * n[2] > 2 ** 31 - 1:
        raise ValueError(f"plan_prefix: shape {tuple(shape)}: three extents in 1..65535 and at most 2^31 - 1 voxels expected")
    b = tuple(int(v) for v in box)
    if len(b) != 6:
        raise ValueError(f"plan_prefix: box {tuple(box)}: (lo0, lo1, lo2, hi0, hi1, hi2) expected")
    if any(b[3 + k] <= b[k] for k in range(3)):
        raise ValueError(f"plan_prefix: empty foreground box {b}: no voxel of the volume is above 0 after the intensity window")
    if any(b[k] < 0 or b[3 + k] > n[k] for k in range(3)):
        raise ValueError(f"plan_prefix: box {b} outside the volume {n}")
    if (affine is None) == (spacing is None and axcodes is None):
        raise ValueError("plan_prefix: give either affine=, or spacing= together with axcodes=")
    if affine is not None:
        perm, sign, zooms = orientation_from_affine(affine)
    else:
        if spacing is None or axcodes is None:
            raise ValueError("plan_prefix: spacing= and axcodes= go together")
        perm, sign = orientation_from_axcodes(axcodes)
        zooms = tuple(float(v) for v in spacing)
        if len(zooms) != 3:
            raise ValueError(f"plan_prefix: spacing {tuple(spacing)}: three voxel sizes expected")
    p = tuple(float(v) for v in pixdim)
    if len(p) != 3 or not all(np.isfinite(v) and v > 0 for v in zooms + p):
        raise ValueError(f"plan_prefix: spacing {zooms} and pixdim {tuple(pixdim)} must be three finite positive values each")
    s = tuple(zooms[perm[a]] for a in range(3))
    e = tuple(b[3 + perm[a]] - b[perm[a]] for a in range(3))
    if pad_to is None:
        front, m = (0, 0, 0), e
    else:
        t = tuple(int(v) for v in pad_to)
        if len(t) != 3 or min(t) < 1:
            raise ValueError(f"plan_prefix: pad_to {tuple(pad_to)}: three positive extents expected")
        front = tuple(max(t[a] - e[a], 0) // 2 for a in range(3))
        m = tuple(max(t[a], e[a]) for a in range(3))
    o = tuple(prefix_out_extent(m[a], s[a], p[a]) for a in range(3))
    if max(m) > 65535 or min(o) < 1 or max(o) > 65535 or o[0] * o[1] * o[2] > 2 ** 31 - 1:
        raise ValueError(f"plan_prefix: padded extents {m} -> output extents {o}: each must be in 1..65535 and the output at most 2^31 - 1 voxels")
    consts, clip = _window_constants(window)
    return PrefixPlan(shape=n, box=b, perm=perm, sign=sign, spacing=s, pixdim=p, pad_front=front, padded_shape=m, out_shape=o,
                      window=consts, clip=clip)


_stream_of = _lib.stream_of


def _refuse_host_memory(dev, who: str):
    """The prefix kernels read device memory: anything but a HIP device is refused (only the tests' emulation library takes host
    pointers), before a host address could reach a launch."""
    if dev.type != "cuda" and not _lib.host_pointers_ok():
        raise ValueError(f"{who}: the data must be on a HIP device, got {dev}")


def _raw_pair(image, label, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """The raw pair on the device: image fp32 [n0, n1, n2], label uint8 (host arrays through ``_as_label_u8``; a device label must be
    uint8 already).  A leading channel axis of 1 is dropped."""
    def squeeze(x):
        return x[0] if x.ndim == 4 and x.shape[0] == 1 else x

    if torch.is_tensor(image) and image.device.type != "cpu":
        image_d = squeeze(image).to(device=device, dtype=torch.float32).contiguous()
    else:
        image_d = torch.as_tensor(np.ascontiguousarray(squeeze(_host_array(image)), dtype=np.float32)).to(device)
    if torch.is_tensor(label) and label.device.type != "cpu":
        if label.dtype != torch.uint8:
            raise ValueError(f"amos_prefix: a label on the device must be uint8, got {label.dtype}")
        label_d = squeeze(label).to(device).contiguous()
    else:
        label_d = torch.as_tensor(np.ascontiguousarray(_as_label_u8(squeeze(_host_array(label))))).to(device)
    if image_d.ndim != 3 or image_d.shape != label_d.shape:
        raise ValueError(f"amos_prefix: image {tuple(image_d.shape)} and label {tuple(label_d.shape)} must be [W,H,D] (or [1,W,H,D]) of one extent")
    return image_d, label_d


def amos_prefix(image, label, device=None, affine=None, spacing=None, axcodes=None, pixdim: Sequence[float] = PREFIX_PIXDIM,
                pad_to: Optional[Sequence[int]] = None, window=PREFIX_WINDOW, out=None):
    """The cached prefix of one case on the device: ``(image_t fp32 [o0, o1, o2], label_t uint8 [o0, o1, o2], plan)``.  ``image`` /
    ``label``: the raw volume ``[n0, n1, n2]`` as read from the file (host arrays or tensors; the label by the rules of
    ``amos_volume_store``) with its ``affine`` (or ``spacing`` and ``axcodes``); the other arguments are ``plan_prefix``'s.  The raw
    pair goes up, ``icl_prefix_box`` finds the foreground box, the six integers are read back ONCE (they size the output; no foreground:
    ``ValueError``), and one ``icl_prefix_resample`` launch writes both outputs.  ``out=(image_t, label_t)``: write into the caller's
    contiguous tensors of exactly the planned shape.  ``device``: default the image's, if it is a device tensor, else ``cuda``."""
    if device is None:
        device = image.device if torch.is_tensor(image) and image.device.type != "cpu" else torch.device("cuda")
    dev = torch.device(device)
    _refuse_host_memory(dev, "amos_prefix")
    image_d, label_d = _raw_pair(image, label, dev)
    n = tuple(int(v) for v in image_d.shape)
    if max(n) > 65535 or n[0] * n[1] * n[2] > 2 ** 31 - 1:
        raise ValueError(f"amos_prefix: extents {n}: each must be below 65,536 and the volume at most 2^31 - 1 voxels")
    consts, clip = _window_constants(window)
    L = _lib.lib()
    stream = _stream_of(dev)
    box_d = torch.empty(6, dtype=torch.int32, device=dev)
    ws = torch.empty(PREFIX_BOX_WS_INTS, dtype=torch.int32, device=dev)
    _lib.check(L.icl_prefix_box(image_d.data_ptr(), *n, (ctypes.c_float * 5)(*consts), int(clip), box_d.data_ptr(), ws.data_ptr(), stream),
               "prefix_box")
    found = [int(v) for v in box_d.cpu()]                                   # the single read-back of a case
    plan = plan_prefix(n, (*found[:3], *(v + 1 for v in found[3:])), affine=affine, spacing=spacing, axcodes=axcodes, pixdim=pixdim,
                       pad_to=pad_to, window=window)
    if out is None:
        image_t = torch.empty(plan.out_shape, dtype=torch.float32, device=dev)
        label_t = torch.empty(plan.out_shape, dtype=torch.uint8, device=dev)
    else:
        image_t, label_t = out
        for name, t, dtype in (("image", image_t, torch.float32), ("label", label_t, torch.uint8)):
            if not torch.is_tensor(t) or t.device.type != dev.type or t.dtype != dtype or tuple(t.shape) != plan.out_shape or not t.is_contiguous():
                raise ValueError(f"amos_prefix: out {name} must be a contiguous {dtype} tensor of shape {plan.out_shape} on {dev}")
    _lib.check(L.icl_prefix_resample(image_d.data_ptr(), label_d.data_ptr(), plan.int_params(), plan.double_params(), plan.window_params(),
                                     int(plan.clip), image_t.data_ptr(), label_t.data_ptr(), stream), "prefix_resample")
    return image_t, label_t, plan


def _case_fields(case) -> tuple:
    """``(image, label, orientation keywords)`` of one raw case: a dictionary with ``image``, ``label`` and ``affine`` (or ``spacing`` and
    ``axcodes``), or an ``(image, label, affine)`` triple."""
    if isinstance(case, dict):
        how = {k: case[k] for k in ("affine", "spacing", "axcodes") if case.get(k) is not None}
        return case["image"], case["label"], how
    if len(case) != 3:
        raise ValueError("a raw case is a dictionary with image, label and affine (or spacing and axcodes), or an (image, label, affine) triple")
    return case[0], case[1], {"affine": case[2]}


def amos_volume_store_from_raw(cases: Iterable, device, pixdim: Sequence[float] = PREFIX_PIXDIM, window=PREFIX_WINDOW):
    """``(store, plans)``: the ``DeviceVolumeStore`` of the training set from RAW cases, what ``CacheDataset`` caches for the AMOS trainer
    (``:86-101``), computed by ``amos_prefix``: the preprocessed volumes never visit the host.  ``cases``: see ``_case_fields``."""
    images, labels, plans = [], [], []
    for case in cases:
        image, label, how = _case_fields(case)
        image_t, label_t, plan = amos_prefix(image, label, device, pixdim=pixdim, window=window, **how)
        images.append(image_t)
        labels.append(label_t)
        plans.append(plan)
    return DeviceVolumeStore.from_device_tensors(images, labels, device), plans


def amos_val_cases_from_raw(cases: Iterable, device, pad_to: Optional[Sequence[int]] = (96, 96, 96), pixdim: Sequence[float] = PREFIX_PIXDIM,
                            window=PREFIX_WINDOW):
    """``(items, plans)``: the validation chain (``:141-154``: the prefix with ``SpatialPadd(96^3)`` before ``Spacingd``) of RAW cases as
    the items ``val_3D.test_all_case_amos`` iterates, ``{'image': [1,1,o0,o1,o2] fp32, 'label': [1,1,o0,o1,o2] uint8}`` on the device
    (batch and channel axes as MONAI's loader of batch size 1 gives them), and the plans ``restore_label`` needs."""
    items, plans = [], []
    for case in cases:
        image, label, how = _case_fields(case)
        image_t, label_t, plan = amos_prefix(image, label, device, pixdim=pixdim, pad_to=pad_to, window=window, **how)
        items.append({"image": image_t[None, None], "label": label_t[None, None]})
        plans.append(plan)
    return items, plans


def restore_label(prediction, plan: PrefixPlan) -> torch.Tensor:
    """A label map on the respaced grid back on the scanner's: what MONAI's ``Invertd`` does to a prediction.  ``prediction``: a uint8
    or int64 tensor of ``plan.out_shape`` (leading axes of 1 are dropped; of an int64 value the low byte is kept) on a HIP device; a host array or CPU tensor is a ``ValueError``.  Returns uint8 ``plan.shape``: 0
    outside the foreground box, inside it the prediction at ``rint(min(max(u * (s / p), 0), o - 1))`` per oriented axis."""
    pred = prediction if torch.is_tensor(prediction) else torch.as_tensor(np.ascontiguousarray(prediction))
    pred = pred.reshape(pred.shape[-3:]) if pred.ndim > 3 and all(v == 1 for v in pred.shape[:-3]) else pred
    if tuple(pred.shape) != plan.out_shape or pred.dtype not in (torch.uint8, torch.int64):
        raise ValueError(f"restore_label: a uint8 or int64 prediction of shape {plan.out_shape} expected, got {tuple(pred.shape)} {pred.dtype}")
    pred = pred.contiguous()
    dev = pred.device
    _refuse_host_memory(dev, "restore_label")
    out = torch.empty(plan.shape, dtype=torch.uint8, device=dev)
    _lib.check(_lib.lib().icl_prefix_restore(pred.data_ptr(), 0 if pred.dtype == torch.uint8 else 1, plan.int_params(), plan.double_params(),
                                             out.data_ptr(), _stream_of(dev)), "prefix_restore")
    return out
