"""Data feed of the 3-D ICL trainers, MI355X-first.

What the reference does (``/root/reference/code/dataloaders/brats2019.py``, used at
``train_inherent_consistent_unet_3D_BraTS.py:66-83``): an h5 volume per index, ``RandomRotFlip -> RandomCrop(96^3) -> ToTensor``
in four host worker processes, batches of labeled + unlabeled indices from ``TwoStreamBatchSampler``.  At >100 volumes/s per GPU a
numpy loader is the bottleneck, and the whole training set is 9 GB of fp32 against 288 GB of HBM, so here

* ``DeviceVolumeStore`` keeps every training volume resident on the GPU (fp32 image + uint8 label),
* ``OnDeviceAugment`` draws the augmentation parameters on the host with the reference's numpy call sequence
  (``:136-139`` then ``:116-118``) and produces the whole batch — rot90, flip, zero padding, crop, ``ToTensor`` casts — with ONE
  gather kernel (``csrc/kernels/datafeed.h``),
* ``TwoStreamBatchSampler`` yields the same index batches as the reference class for the same numpy seed (``:191-237``) and can
  shard every global batch over data-parallel ranks,
* ``BraTS2019`` reads the reference's file layout (``train.txt`` / ``val.txt`` + ``data/<case>.h5``) for callers that want the
  host path (needs h5py, which the reference requires too).
"""
from __future__ import annotations

import ctypes
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch.utils.data import Dataset
from torch.utils.data.sampler import Sampler

from .. import _lib
from .affine import _affine_arguments, _affine_block, _affine_suffixes, _draw_affine
from .intensity import _check_stage, _intensity_rows

FEED_MAX_BATCH = 16         # samples per launch of the 3-D gather entries, icl_crop_rotflip* and icl_volume_feed* (kFeedMaxBatch)


# --------------------------------------------------------------------------------------------------------------------
# index streams
# --------------------------------------------------------------------------------------------------------------------

class _ShuffledStream:
    """Index source that hands out ``count`` indices at a time from successive ``np.random.permutation`` draws.  A new
    permutation is drawn only at the moment the previous one is used up (possibly in the middle of a request), which is when
    the reference's chained generator draws it — the numpy generator is shared with everything else in the process, so the
    moment of every draw is part of the contract."""

    def __init__(self, indices: Sequence[int], endless: bool):
        self.indices = indices
        self.endless = endless
        self.pool = np.empty(0, dtype=np.int64)
        self.pos = 0
        self.drawn = False

    def _refill(self) -> bool:
        if self.drawn and not self.endless:
            return False
        self.pool = np.random.permutation(self.indices)
        self.pos = 0
        self.drawn = True
        return True

    def take(self, count: int) -> Optional[tuple]:
        got = []
        while len(got) < count:
            if self.pos >= len(self.pool) and not self._refill():
                return None            # a single pass ran out: the incomplete tail is dropped
            got.append(self.pool[self.pos])
            self.pos += 1
        return tuple(got)


class TwoStreamBatchSampler(Sampler):
    """Batches of ``batch_size - secondary_batch_size`` primary (labeled) indices followed by ``secondary_batch_size`` secondary
    (unlabeled) ones.  One epoch is a single shuffled pass over the primary indices; the secondary indices come from an endless
    sequence of shuffles (reference: ``dataloaders/brats2019.py:191-237``).  With ``world_size > 1`` every rank draws the same
    global batches (same numpy seed) and keeps elements ``rank::world_size`` of each half, so W ranks together consume exactly
    the batches of one reference process."""

    def __init__(self, primary_indices, secondary_indices, batch_size, secondary_batch_size, rank: int = 0, world_size: int = 1):
        self.primary_indices = primary_indices
        self.secondary_indices = secondary_indices
        self.secondary_batch_size = secondary_batch_size
        self.primary_batch_size = batch_size - secondary_batch_size
        self.rank, self.world_size = rank, world_size
        if not (len(primary_indices) >= self.primary_batch_size > 0):
            raise AssertionError("need at least one full primary batch")
        if not (len(secondary_indices) >= self.secondary_batch_size > 0):
            raise AssertionError("need at least one full secondary batch")
        if self.primary_batch_size % world_size or self.secondary_batch_size % world_size:
            raise AssertionError("the global labeled / unlabeled batch must split evenly over the ranks")

    def __len__(self):
        return len(self.primary_indices) // self.primary_batch_size

    def __iter__(self):
        primary = _ShuffledStream(self.primary_indices, endless=False)
        primary._refill()                                   # the epoch's primary shuffle is drawn here, when iteration is set up ...
        secondary = _ShuffledStream(self.secondary_indices, endless=True)   # ... the first secondary one with the first batch
        return self._batches(primary, secondary)

    def _batches(self, primary, secondary):
        r, w = self.rank, self.world_size
        while True:
            lab = primary.take(self.primary_batch_size)
            if lab is None:
                return
            unl = secondary.take(self.secondary_batch_size)
            yield lab[r::w] + unl[r::w]


# --------------------------------------------------------------------------------------------------------------------
# host dataset (reference file layout)
# --------------------------------------------------------------------------------------------------------------------

class BraTS2019(Dataset):
    """``<base_dir>/train.txt`` | ``val.txt`` list the cases, ``<base_dir>/data/<case>.h5`` holds ``image`` (fp32 [W,H,D]) and
    ``label`` (reference: ``dataloaders/brats2019.py:11-46``).  ``split='test'`` reads ``val.txt`` as the reference does.
    ``read_case`` returns whatever the h5 holds: a multi-modal case is stored channel-first, ``image`` fp32 ``[C,W,H,D]`` (BraTS: FLAIR,
    T1, T1ce, T2) beside ``label`` ``[W,H,D]``, and the transforms below, ``DeviceVolumeStore`` and the validation take that layout."""

    def __init__(self, base_dir=None, split="train", num=None, transform=None):
        self._base_dir = base_dir
        self.transform = transform
        listing = {"train": "train.txt", "test": "val.txt"}[split]
        with open(os.path.join(base_dir, listing)) as f:
            self.image_list = [ln.strip().split(",")[0] for ln in f if ln.strip()]
        if num is not None:
            self.image_list = self.image_list[:num]

    def __len__(self):
        return len(self.image_list)

    def read_case(self, idx) -> Tuple[np.ndarray, np.ndarray]:
        import h5py   # the reference's reader; not installed everywhere, only needed for real data
        with h5py.File(os.path.join(self._base_dir, "data", f"{self.image_list[idx]}.h5"), "r") as h5f:
            return h5f["image"][:], h5f["label"][:].astype(np.uint8)

    def __getitem__(self, idx):
        image, label = self.read_case(idx)
        sample = {"image": image, "label": label}
        return self.transform(sample) if self.transform else sample


# --------------------------------------------------------------------------------------------------------------------
# device-resident volumes + fused augmentation
# --------------------------------------------------------------------------------------------------------------------

class DeviceVolumeStore:
    """All volumes of a split resident in HBM: ``images[i]`` fp32 [W,H,D], ``labels[i]`` uint8 [W,H,D] (the h5 dtypes).

    Multi-modal volumes: an image may be channel-first ``[C,W,H,D]`` (BraTS: FLAIR, T1, T1ce, T2, co-registered) beside ONE label
    ``[W,H,D]``.  All volumes of a store have the same layout and the same C; ``channels`` is C for a 4-D store and 1 for a 3-D one,
    ``multichannel`` says which of the two it is (a ``[1,W,H,D]`` store is 4-D: its batches come from the channel kernel)."""

    MAX_CHANNELS = 16               # kChannelNormMaxChannels: what icl_crop_rotflip_channels takes

    def __init__(self, volumes: Sequence[Tuple[np.ndarray, np.ndarray]], device):
        self.device = torch.device(device)
        self.images: List[torch.Tensor] = []
        self.labels: List[torch.Tensor] = []
        self.channels = 1
        self.multichannel = False
        for image, label in volumes:
            self._admit(tuple(image.shape), tuple(label.shape))
            self.images.append(torch.as_tensor(np.ascontiguousarray(image, dtype=np.float32)).to(self.device))
            self.labels.append(torch.as_tensor(np.ascontiguousarray(label, dtype=np.uint8)).to(self.device))

    def _admit(self, image_shape: tuple, label_shape: tuple):
        """Checks the layout of the next volume against the store's (the first volume decides it)."""
        if len(image_shape) not in (3, 4) or image_shape[-3:] != label_shape:
            raise ValueError("a volume is an (image [W,H,D] or [C,W,H,D], label [W,H,D]) pair")
        multi = len(image_shape) == 4
        channels = image_shape[0] if multi else 1
        if not 1 <= channels <= self.MAX_CHANNELS:
            raise ValueError(f"a volume has 1 to {self.MAX_CHANNELS} channels, got {channels}")
        if self.images and (multi != self.multichannel or channels != self.channels):
            have = f"[{self.channels},W,H,D]" if self.multichannel else "[W,H,D]"
            raise ValueError(f"all volumes of a store have the same channels: the store holds {have} images, got {list(image_shape)}")
        self.multichannel, self.channels = multi, channels

    @classmethod
    def from_dataset(cls, dataset: BraTS2019, device):
        return cls([dataset.read_case(i) for i in range(len(dataset))], device)

    @classmethod
    def from_device_tensors(cls, images: Sequence[torch.Tensor], labels: Sequence[torch.Tensor], device):
        """Adopts volumes that are on ``device`` already (``amos_volume_store_from_raw``): contiguous fp32 ``[W,H,D]`` (or ``[C,W,H,D]``)
        images and uint8 ``[W,H,D]`` labels of the same extents.  Nothing is copied."""
        store = cls([], device)
        if len(images) != len(labels):
            raise ValueError("one label per image")
        for image, label in zip(images, labels):
            ok = (torch.is_tensor(image) and torch.is_tensor(label) and image.ndim in (3, 4) and label.ndim == 3
                  and image.shape[-3:] == label.shape
                  and image.dtype == torch.float32 and label.dtype == torch.uint8 and image.is_contiguous() and label.is_contiguous()
                  and image.device.type == store.device.type and label.device == image.device)
            if not ok:
                raise ValueError("a volume is a contiguous (image fp32 [W,H,D] or [C,W,H,D], label uint8 [W,H,D]) pair of tensors on "
                                 f"{store.device}")
            store._admit(tuple(image.shape), tuple(label.shape))
            store.images.append(image)
            store.labels.append(label)
        return store

    def __len__(self):
        return len(self.images)


def draw_rotflip_crop(shape: Sequence[int], output_size: Sequence[int]) -> List[int]:
    """The random draws of ``RandomRotFlip()`` followed by ``RandomCrop(output_size)`` for one volume of ``shape``, in the
    reference's order (``brats2019.py:136-139``: ``k = randint(0, 4)``, ``axis = randint(0, 2)``; ``:97-118``: padding by
    ``max((out - dim) // 2 + 3, 0)`` on every axis if ANY axis is not larger than the patch, then ``randint(0, dim - out)`` per
    axis).  Returns the 11 integers of one ``icl_crop_rotflip`` parameter row."""
    n0, n1, n2 = (int(v) for v in shape)
    k = int(np.random.randint(0, 4))
    axis = int(np.random.randint(0, 2))
    dims = [n1, n0, n2] if k & 1 else [n0, n1, n2]          # rot90 on axes (0, 1) swaps them for odd k
    pads = [0, 0, 0]
    if any(dims[a] <= output_size[a] for a in range(3)):
        pads = [max((output_size[a] - dims[a]) // 2 + 3, 0) for a in range(3)]
    origin = [int(np.random.randint(0, dims[a] + 2 * pads[a] - output_size[a])) for a in range(3)]
    return [n0, n1, n2, k, axis, *pads, *origin]


class OnDeviceAugment:
    """``Compose([RandomRotFlip(), RandomCrop(patch), ToTensor()])`` + batch collation on the GPU: ``batch(indices)`` returns
    ``{'image': [B,C,*patch] fp32, 'label': [B,*patch] int64}`` like the reference DataLoader's ``sampled_batch`` (C = 1 for a store
    of ``[W,H,D]`` volumes, which goes through ``icl_crop_rotflip`` as ever; a store of ``[C,W,H,D]`` volumes goes through
    ``icl_crop_rotflip_channels``: one launch, one geometry per sample for all of its channels, the label read once).
    ``intensity``: None, or an ``IntensityAugment`` for ``patch_size`` (``dataloaders/intensity.py``; the reference's ``RandomNoise``,
    ``:150-161``, is its noise with ``noise_sigma=0.1, noise_clip=2``): its rows (``intensity_params``: one per sample, or with the
    stage's ``per_channel`` one per sample and channel, sample-major) are drawn after all geometric rows of the batch, from the
    stage's own ``rng``, and it runs in place behind the gather on the same stream.

    **Random rotation and zoom** (MONAI ``RandAffined``, nnU-Net's rotation and scaling; off by default: ``affine_prob=0``), the keywords
    of the AMOS feeds (``affine_prob``, ``rotate_range`` in radians, ``zoom_range``, ``zoom_isotropic``; ``dataloaders/affine.py``), for
    ``[W,H,D]`` and ``[C,W,H,D]`` stores alike.  A sample's affine is drawn from the global ``np.random`` directly after that sample's
    ``draw_rotflip_crop`` (``rand() < affine_prob`` and, only if true, three angles and one or three zooms), and its row then carries the
    nine entries of ``affine_matrix(theta, zoom)`` behind the 11 integers: 20 values.  With ``affine_prob=0`` nothing is drawn for the
    stage, so every seed yields the rows it yielded without it.  The stage rotates and zooms the rotated and flipped volume about the
    patch centre: trilinear for every channel of the image, nearest for the label, zeros outside the volume (DESIGN.md §2 "Affine stage of
    the BraTS feed"; ``tests/crop_affine_ref.py`` restates it in numpy).  A launch of at most 16 samples in which no row has a matrix is
    the launch described above; any other goes through ``icl_crop_rotflip_affine`` (a ``[W,H,D]`` store with ``channels = 1``), which
    computes an output voxel's coordinates, tap offsets and weights once for all channels and the label."""

    def __init__(self, store: DeviceVolumeStore, patch_size: Sequence[int] = (96, 96, 96), intensity=None, affine_prob: float = 0.0,
                 rotate_range=(0, 0, 0), zoom_range=(1.0, 1.0), zoom_isotropic: bool = True):
        self.store = store
        self.patch = tuple(int(v) for v in patch_size)
        _check_stage(intensity, self.patch, "OnDeviceAugment")
        self.intensity = intensity
        self.affine = _affine_arguments(affine_prob, rotate_range, zoom_range, zoom_isotropic)

    def draw(self, indices: Sequence[int]) -> List[list]:
        """The geometric rows of a batch, from the global ``np.random``: per sample ``draw_rotflip_crop`` and directly behind it the
        affine draw (nothing with ``affine_prob == 0``).  11 values, or 20 for a sample that drew an affine."""
        rows = []
        for i in indices:
            row = draw_rotflip_crop(self.store.images[i].shape[-3:], self.patch)
            rows.append(row + list(_draw_affine(np.random, *self.affine)))
        return rows

    def batch(self, indices: Sequence[int], params: Optional[Sequence[Sequence[float]]] = None, intensity_params=None):
        st = self.store
        n = len(indices)
        if params is None:
            params = self.draw(indices)
        suffixes = _affine_suffixes("OnDeviceAugment.batch", params, 11, "one parameter row of 11 values per index")
        channels = st.channels
        intensity_params = _intensity_rows(self.intensity, self.patch, n, intensity_params, "OnDeviceAugment.batch", channels)
        dev = st.device
        image = torch.empty((n, channels) + self.patch, dtype=torch.float32, device=dev)
        label = torch.empty((n,) + self.patch, dtype=torch.int64, device=dev)
        L = _lib.lib()
        stream = _lib.stream_of(dev)
        for lo in range(0, n, FEED_MAX_BATCH):            # every entry takes up to FEED_MAX_BATCH samples per launch
            chunk = list(indices[lo:lo + FEED_MAX_BATCH])
            m = len(chunk)
            ptrs = ctypes.c_void_p * m
            flat = (ctypes.c_int32 * (11 * m))(*[int(v) for row in params[lo:lo + m] for v in row[:11]])
            images, labels = ptrs(*[st.images[i].data_ptr() for i in chunk]), ptrs(*[st.labels[i].data_ptr() for i in chunk])
            affine = _affine_block(suffixes[lo:lo + m])
            if st.multichannel or affine is not None:
                for i, row in zip(chunk, params[lo:lo + m]):      # the kernel strides the channels by the row's extents
                    if tuple(int(v) for v in row[:3]) != tuple(st.images[i].shape[-3:]):
                        raise ValueError(f"OnDeviceAugment.batch: the row of volume {i} names the extents {tuple(row[:3])}, the volume "
                                         f"has {tuple(st.images[i].shape[-3:])}")
            if affine is not None:
                _lib.check(L.icl_crop_rotflip_affine(images, labels, flat, affine, m, channels, image[lo:].data_ptr(), label[lo:].data_ptr(),
                                                     *self.patch, stream), "crop_rotflip_affine")
            elif st.multichannel:
                _lib.check(L.icl_crop_rotflip_channels(images, labels, flat, m, channels, image[lo:].data_ptr(), label[lo:].data_ptr(),
                                                       *self.patch, stream), "crop_rotflip_channels")
            else:
                _lib.check(L.icl_crop_rotflip(images, labels, flat, m, image[lo:].data_ptr(), label[lo:].data_ptr(), *self.patch, stream),
                           "crop_rotflip")
        if intensity_params is not None:
            self.intensity.apply(image, intensity_params)
        return {"image": image, "label": label}


# --------------------------------------------------------------------------------------------------------------------
# channel-wise normalisation of a resident volume
# --------------------------------------------------------------------------------------------------------------------

NORM_MASKS = {"nonzero": 0, "positive": 1, "all": 2}
NORM_APPLY = {"mask": 0, "all": 1}
NORM_WS_DOUBLES = 16 * 256 * 2      # kChannelNormMaxChannels * kChannelNormBlocks * 2


def _norm_volume(volume, mask: str, who: str):
    if mask not in NORM_MASKS:
        raise ValueError(f"{who}: mask {mask!r} must be one of {sorted(NORM_MASKS)}")
    if not torch.is_tensor(volume) or volume.dtype != torch.float32 or not volume.is_contiguous() or volume.ndim not in (3, 4) \
            or volume.numel() < 1:
        got = f"{tuple(volume.shape)} {volume.dtype}" if torch.is_tensor(volume) else type(volume).__name__
        raise ValueError(f"{who}: a contiguous fp32 tensor [C,W,H,D] or [W,H,D] expected, got {got}")
    if volume.device.type != "cuda" and not _lib.host_pointers_ok():
        raise ValueError(f"{who}: the volume must be on a HIP device, got {volume.device}")
    channels = int(volume.shape[0]) if volume.ndim == 4 else 1
    if not 1 <= channels <= DeviceVolumeStore.MAX_CHANNELS:
        raise ValueError(f"{who}: 1 to {DeviceVolumeStore.MAX_CHANNELS} channels, got {channels}")
    return channels, volume.numel() // channels


def channel_norm_stats(volume: torch.Tensor, mask: str = "nonzero") -> torch.Tensor:
    """Per channel of a device fp32 ``[C,W,H,D]`` (or ``[W,H,D]``) volume: a device fp64 tensor ``[C,4]`` = ``(count, mean, std, 0)``
    of the voxels in ``mask`` (``"nonzero"``: ``x != 0``; ``"positive"``: ``x > 0``; ``"all"``), the POPULATION standard deviation,
    in double and in two passes (the mean, then the sum of ``(x - mean)**2``), every sum in a fixed order without atomics
    (``channel_norm_partial_kernel`` in ``csrc/kernels/datafeed.h``).  An empty mask gives four zeros.  Nothing is read back."""
    channels, voxels = _norm_volume(volume, mask, "channel_norm_stats")
    dev = volume.device
    stats = torch.empty((channels, 4), dtype=torch.float64, device=dev)
    ws = torch.empty(NORM_WS_DOUBLES, dtype=torch.float64, device=dev)
    stream = _lib.stream_of(dev)
    _lib.check(_lib.lib().icl_channel_norm_stats(volume.data_ptr(), channels, voxels, NORM_MASKS[mask], stats.data_ptr(), ws.data_ptr(),
                                                 stream), "channel_norm_stats")
    return stats


def normalize_channels_(volume: torch.Tensor, mask: str = "nonzero", apply_to: str = "mask") -> torch.Tensor:
    """Channel-wise z-score of a device fp32 ``[C,W,H,D]`` (or ``[W,H,D]``) volume IN PLACE, before it enters a ``DeviceVolumeStore``;
    returns ``volume``.  ``("nonzero", "mask")`` restates MONAI's ``NormalizeIntensityd(nonzero=True, channel_wise=True)``, the first
    transform of every multi-modal BraTS recipe; ``("positive", "all")`` restates the statistics and the formula of the reference's
    ``itensity_normalize_one_volume`` (``dataloaders/brats_proprecessing.py:62-78``).  Per channel: ``m, s = channel_norm_stats``'s
    mean and std rounded to fp32, ``s = 1`` where it is 0, then ``x = (x - m) / s`` in fp32 (a true subtraction, a true division) on
    the voxels of the mask (``apply_to="mask"``) or on every voxel (``"all"``).  A channel with an empty mask is left untouched.
    Everything stays on the stream; the host reads nothing back.  DESIGN.md §2 "Multi-modal feed" has the definition rounding by
    rounding; ``tests/multimodal_feed_ref.py`` restates it in numpy, and the result equals that bit for bit.  **Parity with MONAI's own
    code is unpinned**: MONAI is not installed where this package is built and tested."""
    if apply_to not in NORM_APPLY:
        raise ValueError(f"normalize_channels_: apply_to {apply_to!r} must be one of {sorted(NORM_APPLY)}")
    channels, voxels = _norm_volume(volume, mask, "normalize_channels_")
    stats = channel_norm_stats(volume, mask)
    dev = volume.device
    stream = _lib.stream_of(dev)
    _lib.check(_lib.lib().icl_channel_norm_apply(volume.data_ptr(), channels, voxels, NORM_MASKS[mask], NORM_APPLY[apply_to],
                                                 stats.data_ptr(), stream), "channel_norm_apply")
    return volume


# --------------------------------------------------------------------------------------------------------------------
# host transforms (the reference's numpy path, for callers that keep its DataLoader: same sample dicts, same random draws)
# --------------------------------------------------------------------------------------------------------------------

def _pad_to_patch(arrays, output_size):
    """Zero-pad every array on both sides of each spatial axis (its last three: a channel-first 4-D image keeps its channel axis) by
    ``max((out - dim) // 2 + 3, 0)`` when ANY axis of the volume does not exceed the patch (brats2019.py:53-62,97-109)."""
    shape = arrays[0].shape[-3:]
    if all(shape[a] > output_size[a] for a in range(3)):
        return arrays
    widths = [(max((output_size[a] - shape[a]) // 2 + 3, 0),) * 2 for a in range(3)]
    return [np.pad(v, [(0, 0)] * (v.ndim - 3) + widths, mode="constant", constant_values=0) for v in arrays]


def _window(arrays, origin, output_size):
    sl = tuple(slice(origin[a], origin[a] + output_size[a]) for a in range(3))
    return [v[(Ellipsis,) + sl] for v in arrays]


class RandomRotFlip:
    """k = randint(0, 4) quarter turns in the (0, 1) plane, then a flip along axis randint(0, 2) (brats2019.py:128-144).  A
    channel-first 4-D ``image`` ``[C,W,H,D]`` beside a 3-D ``label`` is turned and flipped in its spatial axes (the first two of its
    last three), all channels alike; the draws are the same two."""

    def __call__(self, sample):
        k = np.random.randint(0, 4)
        axis = np.random.randint(0, 2)
        out = dict(sample)
        for key in ("image", "label"):
            v = sample[key]
            lead = v.ndim - 3                                # 1 for a channel-first image, else 0
            out[key] = np.flip(np.rot90(v, k, axes=(lead, lead + 1)), axis=lead + axis).copy()
        return out


class RandomCrop:
    """Patch at a uniformly drawn origin, after padding small volumes (brats2019.py:80-127; the ``sdf`` channel is carried along
    when ``with_sdf``).  Padding and window act on the last three axes, so a channel-first 4-D ``image`` keeps its channels."""

    def __init__(self, output_size, with_sdf=False):
        self.output_size = output_size
        self.with_sdf = with_sdf

    def __call__(self, sample):
        keys = ["image", "label"] + (["sdf"] if self.with_sdf else [])
        arrays = _pad_to_patch([sample[k] for k in keys], self.output_size)
        origin = [np.random.randint(0, arrays[0].shape[-3:][a] - self.output_size[a]) for a in range(3)]
        return dict(zip(keys, _window(arrays, origin, self.output_size)))


class CenterCrop:
    """Centred patch, same padding rule (brats2019.py:49-77), on the last three axes."""

    def __init__(self, output_size):
        self.output_size = output_size

    def __call__(self, sample):
        arrays = _pad_to_patch([sample["image"], sample["label"]], self.output_size)
        origin = [int(round((arrays[0].shape[-3:][a] - self.output_size[a]) / 2.)) for a in range(3)]
        image, label = _window(arrays, origin, self.output_size)
        return {"image": image, "label": label}


class ToTensor:
    """image -> fp32 tensor [1,W,H,D], label -> int64 tensor (brats2019.py:177-189).  A 4-D image is channel-first already and gets
    no new axis: [C,W,H,D]."""

    def __call__(self, sample):
        image = np.ascontiguousarray(sample["image"], dtype=np.float32)
        if image.ndim == 3:
            image = image[None]
        out = {"image": torch.from_numpy(image), "label": torch.from_numpy(np.ascontiguousarray(sample["label"])).long()}
        if "onehot_label" in sample:
            out["onehot_label"] = torch.from_numpy(sample["onehot_label"]).long()
        return out
