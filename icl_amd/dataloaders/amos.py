"""Data feed of the 3-D AMOS trainer on the device (``train_inherent_consistent_unet_3D_AMOS22.py``).

What the reference does (``:84-138,182-197``): MONAI dictionary transforms in a ``CacheDataset`` behind a ``ThreadDataLoader``.
The deterministic prefix (``LoadImaged … Spacingd``, ``:86-101``) is computed once and cached; the random tail (``:102-133``) runs on
host threads for every sample of every batch:

    RandSpatialCropd(roi 96^3, random_size=False) -> SpatialPadd(96^3) -> RandFlipd(axis 0) -> RandFlipd(axis 1) -> RandFlipd(axis 2)
    -> RandRotate90d(max_k=3) -> RandShiftIntensityd(offsets 0.10)

Here the cached volumes stay resident in HBM (``DeviceVolumeStore``, filled by ``amos_volume_store``), the host draws the random
parameters of a batch (``draw_amos_params``) and ONE gather kernel (``volume_feed_kernel`` in ``csrc/kernels/datafeed.h``, through
``icl_volume_feed``) produces the batch.  ``AMOSDeviceLoader`` stands where the ``ThreadDataLoader`` stood.  The cached prefix stays
MONAI's: it needs NIfTI affines and is not restated.

**Parity with MONAI's own code is unpinned.**  MONAI is not installed where this package is built and tested, so the transform
semantics are restated from MONAI 1.0.1's published definitions (as the window grid and the Gaussian map of ``val_3D`` are) and no golden
vector of MONAI's output exists.  What the tests pin is the kernel against a numpy restatement of the forward chain
(``tests/amos_feed_ref.py``) and the order and number of the random draws documented at ``draw_amos_params``.  MONAI gives every
transform a generator of its own; here one generator serves all of them, so the batches are distributed like MONAI's, not equal to them.

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
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _lib
from .brats2019 import DeviceVolumeStore

FEED_MAX_BATCH = 16         # icl_volume_feed takes up to 16 samples per launch (kFeedMaxBatch)


def draw_amos_params(shape: Sequence[int], roi: Sequence[int], rng=np.random, flip_prob: float = 0.10, rot_prob: float = 0.10,
                     max_k: int = 3, shift_offset: float = 0.10, shift_prob: float = 0.50, scale_factor: float = 0.0,
                     scale_prob: float = 0.0) -> tuple:
    """The random draws of the AMOS trainer's transforms (``:102-133``) for one volume of ``shape``, from ``rng`` (``np.random`` or a
    ``RandomState``), in this fixed order:

    1. crop (``RandSpatialCrop``, ``random_size=False``): the size is ``s = min(roi, n)`` per axis; per axis, in order,
       ``origin = rng.randint(0, n - s + 1)`` ONLY IF ``n > s``, otherwise the origin is 0 and nothing is drawn;
    2. pad (``SpatialPad``, symmetric): ``w = roi - s``, ``w // 2`` on the left, the rest on the right; nothing is drawn;
    3. flips: for axis 0, 1, 2 in turn, ``rng.rand() < flip_prob``;
    4. rotation: ``rng.rand() < rot_prob``; ONLY IF true, ``k = rng.randint(max_k) + 1`` (otherwise ``k = 0``);
    5. scale (``RandScaleIntensity``; off by default — the AMOS trainer has none, ``utils/data_utils.py:98`` has one): with
       ``scale_prob == 0`` nothing is drawn at all; otherwise ``rng.rand() < scale_prob`` and, only if true,
       ``mul = float32(1 + rng.uniform(-scale_factor, scale_factor))``;
    6. shift (``RandShiftIntensity``): ``rng.rand() < shift_prob``; ONLY IF true, ``add = float32(rng.uniform(-o, o))``.

    Returns one ``icl_volume_feed`` parameter row: 14 integers ``(n0, n1, n2, c0, c1, c2, s0, s1, s2, l0, l1, l2, flip mask, k)``
    followed by the two floats ``(mul, add)``."""
    n = [int(v) for v in shape]
    r = [int(v) for v in roi]
    if len(n) != 3 or len(r) != 3 or min(n) < 1 or min(r) < 1:
        raise ValueError(f"draw_amos_params: shape {tuple(shape)} and roi {tuple(roi)} must be three positive extents each")
    size = [min(r[a], n[a]) for a in range(3)]
    origin = [int(rng.randint(0, n[a] - size[a] + 1)) if n[a] > size[a] else 0 for a in range(3)]
    left = [(r[a] - size[a]) // 2 for a in range(3)]
    return (*n, *origin, *size, *left, *_draw_tail(rng, flip_prob, rot_prob, max_k, shift_offset, shift_prob, scale_factor, scale_prob))


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


class OnDeviceAugmentAMOS:
    """The random transforms of the AMOS trainer (``:102-133``) + batch collation on the GPU.  ``batch(indices)`` returns
    ``{'image': [B,1,*roi] fp32, 'label': [B,1,*roi] int64}``: the label carries MONAI's channel axis, so the trainer's
    ``label_batch[:labeled_bs].squeeze(1).long()`` and ``.long()`` (``:225-227``) work unchanged.  Difference to the reference: its
    loader yields a FLOAT32 label there (``ToTensord`` is given the image only and ``LoadImaged`` loads float32); here it is int64
    already and the ``.long()`` calls are no-ops.

    The keyword arguments are those of ``draw_amos_params`` (``flip_prob``, ``rot_prob``, ``max_k``, ``shift_offset``, ``shift_prob``,
    ``scale_factor``, ``scale_prob``) plus ``rng`` (default: numpy's global generator)."""

    def __init__(self, store: DeviceVolumeStore, roi: Sequence[int] = (96, 96, 96), rng=np.random, **probabilities):
        self.store = store
        self.roi = tuple(int(v) for v in roi)
        if len(self.roi) != 3 or min(self.roi) < 1:
            raise ValueError(f"OnDeviceAugmentAMOS: roi {tuple(roi)}")
        self.rng = rng
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

    def batch(self, indices: Sequence[int], params: Optional[Sequence[Sequence[float]]] = None, out=None):
        """One batch for the volumes ``indices`` of the store.  ``params``: one ``draw_amos_params`` row per index (drawn here when
        not given).  ``out=(image, label)``: write into the caller's tensors — for example ``ICLTrainer.static_vol`` /
        ``static_lab`` after ``capture()``, so that a captured step needs no extra copy — and return views of them; shape
        (``[B,1,*roi]``; the label may also be ``[B,*roi]``), dtype, device and contiguity are checked.  More than 16 indices are
        handled as chunks of 16."""
        st = self.store
        indices = [int(i) for i in indices]
        n = len(indices)
        if n < 1:
            raise ValueError("OnDeviceAugmentAMOS.batch: no indices")
        if params is None:
            params = self.draw(indices)
        if len(params) != n or any(len(row) != 16 for row in params):
            raise ValueError("OnDeviceAugmentAMOS.batch: one parameter row of 16 values per index")
        for i, row in zip(indices, params):
            if tuple(int(v) for v in row[:3]) != tuple(st.images[i].shape):
                raise ValueError(f"OnDeviceAugmentAMOS.batch: parameter row for extents {tuple(row[:3])}, volume {i} is {tuple(st.images[i].shape)}")
            if int(row[13]) & 1 and self.roi[0] != self.roi[1]:
                raise ValueError(f"OnDeviceAugmentAMOS.batch: k = {int(row[13])} with roi {self.roi}: an odd quarter turn needs roi[0] == roi[1]")
        image, label = self._outputs(n, out)
        dev = st.device
        per = self.roi[0] * self.roi[1] * self.roi[2]
        flat_image, flat_label = image.view(n, per), label.view(n, per)
        L = _lib.lib()
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream) if dev.type == "cuda" else None
        for lo in range(0, n, FEED_MAX_BATCH):
            chunk = indices[lo:lo + FEED_MAX_BATCH]
            m = len(chunk)
            ptrs = ctypes.c_void_p * m
            ints = (ctypes.c_int32 * (14 * m))(*[int(v) for row in params[lo:lo + m] for v in row[:14]])
            floats = (ctypes.c_float * (2 * m))(*[float(v) for row in params[lo:lo + m] for v in row[14:]])
            _lib.check(L.icl_volume_feed(ptrs(*[st.images[i].data_ptr() for i in chunk]), ptrs(*[st.labels[i].data_ptr() for i in chunk]),
                                         ints, floats, m, flat_image[lo:].data_ptr(), flat_label[lo:].data_ptr(), *self.roi, stream),
                       "volume_feed")
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
    65,536 or more (MONAI's ``uint16`` centres) or more than 2^31 - 1 voxels is refused."""

    def __init__(self, store: DeviceVolumeStore, image_threshold: float = 0.0):
        self.store = store
        self.image_threshold = float(image_threshold)
        self.fg: List[torch.Tensor] = []
        self.bg: List[torch.Tensor] = []
        dev = store.device
        L = _lib.lib()
        tile = rank_tile()
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream) if dev.type == "cuda" else None
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
    3. then, for crop 0, 1, ..., the tail draws, steps 3-6 of ``draw_amos_params`` (flips, rotation, scale, shift).

    The crop has the size ``s = min(roi, n)`` and the origin ``clamp(centre - s // 2, 0, n - s)`` per axis (``correct_crop_centers``
    followed by ``SpatialCrop(roi_center, roi_size)``); the device computes it from the rank, so the origin fields of a row are unused
    (0).  Returns ``num_samples`` rows: the 16 values of a ``draw_amos_params`` row followed by ``(kind, rank)``, ``kind`` being
    ``KIND_FG`` (0) or ``KIND_BG`` (1).  The keyword arguments are the probabilities of ``draw_amos_params``."""
    n = [int(v) for v in shape]
    r = [int(v) for v in roi]
    if len(n) != 3 or len(r) != 3 or min(n) < 1 or min(r) < 1:
        raise ValueError(f"draw_posneg_params: shape {tuple(shape)} and roi {tuple(roi)} must be three positive extents each")
    if pos < 0 or neg < 0 or pos + neg == 0:
        raise ValueError(f"draw_posneg_params: pos = {pos} and neg = {neg} must be non-negative and not both 0")
    num_samples, n_fg, n_bg = int(num_samples), int(n_fg), int(n_bg)
    if num_samples < 1 or n_fg < 0 or n_bg < 0:
        raise ValueError(f"draw_posneg_params: num_samples {num_samples}, n_fg {n_fg}, n_bg {n_bg}")
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
    return [(*n, 0, 0, 0, *size, *left, *_draw_tail(rng, *tail), kind, rank) for kind, rank in centres]


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
                 num_samples: int = 4, rng=np.random, **probabilities):
        super().__init__(store, roi, rng, **probabilities)
        if index.store is not store or len(index) != len(store):
            raise ValueError("OnDeviceAugmentPosNeg: the ForegroundIndex was not built from this store")
        self.index = index
        self.pos, self.neg, self.num_samples = pos, neg, int(num_samples)
        draw_posneg_params((1, 1, 1), self.roi, 1, 1, np.random.RandomState(0), pos, neg, self.num_samples, **probabilities)

    def draw(self, indices: Sequence[int]) -> List[tuple]:
        ix = self.index
        return [row for i in indices for row in draw_posneg_params(self.store.images[i].shape, self.roi, ix.n_fg[i], ix.n_bg[i], self.rng,
                                                                   self.pos, self.neg, self.num_samples, **self.probabilities)]

    def batch(self, indices: Sequence[int], params: Optional[Sequence[Sequence[float]]] = None, out=None):
        """One batch of ``len(indices) * num_samples`` samples.  ``params``: ``num_samples`` ``draw_posneg_params`` rows per index,
        volume-major (drawn here when not given); a rank at or past the length of its list is refused here, since only the host
        knows the lengths.  ``out=(image, label)`` as in ``OnDeviceAugmentAMOS.batch``.  More than 16 samples go as chunks of 16."""
        st, ix, k = self.store, self.index, self.num_samples
        indices = [int(i) for i in indices]
        if len(indices) < 1:
            raise ValueError("OnDeviceAugmentPosNeg.batch: no indices")
        if params is None:
            params = self.draw(indices)
        sample_of = [i for i in indices for _ in range(k)]          # the volume of every sample
        n = len(sample_of)
        if len(params) != n or any(len(row) != 18 for row in params):
            raise ValueError(f"OnDeviceAugmentPosNeg.batch: {k} parameter rows of 18 values per index")
        for i, row in zip(sample_of, params):
            if tuple(int(v) for v in row[:3]) != tuple(st.images[i].shape):
                raise ValueError(f"OnDeviceAugmentPosNeg.batch: parameter row for extents {tuple(row[:3])}, volume {i} is {tuple(st.images[i].shape)}")
            if int(row[13]) & 1 and self.roi[0] != self.roi[1]:
                raise ValueError(f"OnDeviceAugmentPosNeg.batch: k = {int(row[13])} with roi {self.roi}: an odd quarter turn needs roi[0] == roi[1]")
            kind, rank = int(row[16]), int(row[17])
            if kind not in (KIND_FG, KIND_BG):
                raise ValueError(f"OnDeviceAugmentPosNeg.batch: kind {kind} (0 foreground, 1 background)")
            total = ix.n_fg[i] if kind == KIND_FG else ix.n_bg[i]
            if not 0 <= rank < total:
                raise ValueError(f"OnDeviceAugmentPosNeg.batch: rank {rank} outside the {'foreground' if kind == KIND_FG else 'background'} "
                                 f"list of volume {i} ({total} voxels)")
        image, label = self._outputs(n, out)
        dev = st.device
        per = self.roi[0] * self.roi[1] * self.roi[2]
        flat_image, flat_label = image.view(n, per), label.view(n, per)
        origins = torch.empty((n, 3), dtype=torch.int32, device=dev)
        L = _lib.lib()
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream) if dev.type == "cuda" else None
        for lo in range(0, n, FEED_MAX_BATCH):
            chunk = sample_of[lo:lo + FEED_MAX_BATCH]
            rows = params[lo:lo + FEED_MAX_BATCH]
            m = len(chunk)
            ptrs = ctypes.c_void_p * m
            images, labels = ptrs(*[st.images[i].data_ptr() for i in chunk]), ptrs(*[st.labels[i].data_ptr() for i in chunk])
            select = (ctypes.c_int32 * (8 * m))(*[int(v) for row in rows for v in (*row[:3], row[16], row[17], *row[6:9])])
            _lib.check(L.icl_rank_select(images, labels, ptrs(*[ix.fg[i].data_ptr() for i in chunk]), ptrs(*[ix.bg[i].data_ptr() for i in chunk]),
                                         select, ix.image_threshold, m, origins[lo:].data_ptr(), stream), "rank_select")
            ints = (ctypes.c_int32 * (14 * m))(*[int(v) for row in rows for v in row[:14]])
            floats = (ctypes.c_float * (2 * m))(*[float(v) for row in rows for v in row[14:16]])
            _lib.check(L.icl_volume_feed_origins(images, labels, ints, floats, m, origins[lo:].data_ptr(), flat_image[lo:].data_ptr(),
                                                 flat_label[lo:].data_ptr(), *self.roi, stream), "volume_feed_origins")
        return {"image": image, "label": label.view((n, 1) + self.roi)}


class AMOSDeviceLoader:
    """Stands where the AMOS trainer's ``ThreadDataLoader(train_ds, batch_sampler=batch_sampler, …)`` stood (``:196-197``): an
    iterable with ``__len__`` that yields ``augment.batch(indices)`` for the index batches of ``batch_sampler``
    (``TwoStreamBatchSampler``), so ``for i_batch, sampled_batch in enumerate(train_loader)`` runs as written and the loop's ``.cuda()``
    calls are no-ops.  ``augment`` may be an ``OnDeviceAugmentPosNeg``: a batch then holds ``num_samples`` crops per index."""

    def __init__(self, augment: OnDeviceAugmentAMOS, batch_sampler):
        self.augment = augment
        self.batch_sampler = batch_sampler

    def __len__(self):
        return len(self.batch_sampler)

    def __iter__(self):
        for indices in self.batch_sampler:
            yield self.augment.batch(list(indices))
