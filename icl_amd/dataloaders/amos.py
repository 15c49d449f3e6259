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
    return (*n, *origin, *size, *left, flip, k, float(mul), float(add))


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
                raise ValueError(f"OnDeviceAugmentAMOS.batch: out {name} must be a contiguous {dtype} tensor of shape "
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


class AMOSDeviceLoader:
    """Stands where the AMOS trainer's ``ThreadDataLoader(train_ds, batch_sampler=batch_sampler, …)`` stood (``:196-197``): an
    iterable with ``__len__`` that yields ``augment.batch(indices)`` for the index batches of ``batch_sampler``
    (``TwoStreamBatchSampler``), so ``for i_batch, sampled_batch in enumerate(train_loader)`` runs as written and the loop's ``.cuda()``
    calls are no-ops."""

    def __init__(self, augment: OnDeviceAugmentAMOS, batch_sampler):
        self.augment = augment
        self.batch_sampler = batch_sampler

    def __len__(self):
        return len(self.batch_sampler)

    def __iter__(self):
        for indices in self.batch_sampler:
            yield self.augment.batch(list(indices))
