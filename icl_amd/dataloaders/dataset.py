"""Data feed of the 2-D ICL trainers, MI355X-first (the slice counterpart of ``brats2019.py``).

What the reference does (``/root/reference/code/dataloaders/dataset.py``, used at ``train_inherent_consistent_unet_2D.py:17,70-77``
and ``..._swinunet_2D.py``): an h5 slice per index, ``RandomGenerator(patch)`` — maybe rot90 + flip, else maybe
``scipy.ndimage.rotate`` by an integer angle, then two ``scipy.ndimage.zoom`` calls to the patch size, all ``order=0`` — per sample in
eight host worker processes, 16 or 24 samples per step.  Next to a GPU step of a few milliseconds that loader is the bottleneck, and
the ACDC training set is about 1,300 slices of roughly 256 x 216 fp32, a few hundred MB against 288 GB of HBM, so here

* ``DeviceSliceStore`` keeps every training slice resident on the GPU (fp32 image + uint8 label, extents free per slice),
* ``OnDeviceAugment2D`` draws the parameters on the host with the reference's call sequence (``draw_generator``: Python's ``random``
  AND numpy's global generator, ``:156-159``, ``:76-78``, ``:89``) and produces the whole batch with ONE gather kernel
  (``slice_augment_kernel`` in ``csrc/kernels/datafeed.h``): two nearest-neighbour samplings compose into one gather, and every
  coordinate is formed in fp64 with scipy's own products and sums, so the batch equals the reference's bit for bit,
* ``TwoStreamBatchSampler`` is the class of ``brats2019.py`` (the reference's two modules carry the same sampler; rank sharding
  included),
* ``BaseDataSets``, ``RandomGenerator``, ``random_rot_flip``, ``random_rotate`` are the host path for callers that keep the
  reference's ``DataLoader``: same sample dicts, dtypes and draws (needs h5py for real data, which the reference requires too).

Not here: ``CTATransform`` / ``WeakStrongAugment`` / ``color_jitter`` (``:95-144,169-202``), PIL / torchvision policies no ICL trainer
uses; ``BaseDataSets`` refuses ``ops_weak`` / ``ops_strong``.
"""
from __future__ import annotations

import ctypes
import random
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch.utils.data import Dataset

from .. import _lib
from .brats2019 import TwoStreamBatchSampler  # noqa: F401  (re-exported: `from dataloaders.dataset import TwoStreamBatchSampler`)

BRANCH_NONE, BRANCH_ROTFLIP, BRANCH_ROTATE = 0, 1, 2
SLICE_MAX_BATCH = 32        # icl_slice_augment takes up to 32 samples per launch (kSliceMaxBatch)


# --------------------------------------------------------------------------------------------------------------------
# host dataset (reference file layout)
# --------------------------------------------------------------------------------------------------------------------

class BaseDataSets(Dataset):
    """``<base_dir>/train_slices.list`` + ``slices/<case>.h5`` (``split='train'``: one slice per item, transformed) or
    ``val_test.list`` + ``volumes/<case>.h5`` (``split='val_test'``: one untransformed volume per item); every sample carries its
    ``idx`` (reference: ``dataloaders/dataset.py:20-72``).  ``num`` truncates the training list only, as in the reference."""

    def __init__(self, base_dir=None, split="train", num=None, transform=None, ops_weak=None, ops_strong=None):
        if ops_weak or ops_strong:
            raise NotImplementedError("BaseDataSets: ops_weak / ops_strong select the CTAugment policies (CTATransform), which this "
                                      "package does not provide; the ICL trainers pass neither")
        self._base_dir = base_dir
        self.split = split
        self.transform = transform
        self.sample_list: List[str] = []
        listing = {"train": "train_slices.list", "val_test": "val_test.list"}.get(split)
        if listing is not None:
            with open(self._base_dir + "/" + listing, "r") as f:
                self.sample_list = [item.replace("\n", "") for item in f.readlines()]
        if num is not None and self.split == "train":
            self.sample_list = self.sample_list[:num]
        print("total {} samples".format(len(self.sample_list)))

    def __len__(self):
        return len(self.sample_list)

    def read_case(self, idx) -> Tuple[np.ndarray, np.ndarray]:
        import h5py   # the reference's reader; not installed everywhere, only needed for real data
        folder = "slices" if self.split == "train" else "volumes"
        with h5py.File(self._base_dir + "/{}/{}.h5".format(folder, self.sample_list[idx]), "r") as h5f:
            return h5f["image"][:], h5f["label"][:]

    def __getitem__(self, idx):
        image, label = self.read_case(idx)
        sample = {"image": image, "label": label}
        if self.split == "train":
            sample = self.transform(sample)
        sample["idx"] = idx
        return sample


# --------------------------------------------------------------------------------------------------------------------
# host transforms (the reference's scipy path: same sample dicts, same random draws)
# --------------------------------------------------------------------------------------------------------------------

def random_rot_flip(image, label=None):
    """``k = randint(0, 4)`` quarter turns, then a flip along ``randint(0, 2)`` (dataset.py:75-85)."""
    k = np.random.randint(0, 4)
    image = np.rot90(image, k)
    axis = np.random.randint(0, 2)
    image = np.flip(image, axis=axis).copy()
    if label is None:
        return image
    label = np.flip(np.rot90(label, k), axis=axis).copy()
    return image, label


def random_rotate(image, label):
    """Rotation about the centre by ``randint(-20, 20)`` degrees, nearest neighbour, same extent (dataset.py:88-92)."""
    from scipy import ndimage
    angle = np.random.randint(-20, 20)
    image = ndimage.rotate(image, angle, order=0, reshape=False)
    label = ndimage.rotate(label, angle, order=0, reshape=False)
    return image, label


class RandomGenerator:
    """dataset.py:147-166: image -> fp32 tensor [1, O0, O1], label -> uint8 tensor [O0, O1] (the trainer calls ``.long()``)."""

    def __init__(self, output_size):
        self.output_size = output_size

    def __call__(self, sample):
        from scipy.ndimage import zoom
        image, label = sample["image"], sample["label"]
        if random.random() > 0.5:
            image, label = random_rot_flip(image, label)
        elif random.random() > 0.5:
            image, label = random_rotate(image, label)
        x, y = image.shape
        image = zoom(image, (self.output_size[0] / x, self.output_size[1] / y), order=0)
        label = zoom(label, (self.output_size[0] / x, self.output_size[1] / y), order=0)
        image = torch.from_numpy(image.astype(np.float32)).unsqueeze(0)
        label = torch.from_numpy(label.astype(np.uint8))
        return {"image": image, "label": label}


# --------------------------------------------------------------------------------------------------------------------
# device-resident slices + fused RandomGenerator
# --------------------------------------------------------------------------------------------------------------------

def zoom_factor(n_in: int, n_out: int) -> float:
    """The coordinate step of ``scipy.ndimage.zoom(x, n_out / n_in, order=0)`` along one axis, ``(n_in - 1) / (n_out - 1)`` in
    double; scipy derives the output extent as ``round(n_in * (n_out / n_in))``, which must give ``n_out`` back."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 2:
        raise ValueError(f"zoom {n_in} -> {n_out}: the source extent must be >= 1 and the output extent >= 2")
    if int(round(n_in * (n_out / n_in))) != n_out:
        raise AssertionError(f"zoom {n_in} -> {n_out}: scipy would produce {int(round(n_in * (n_out / n_in)))} elements")
    return float(n_in - 1) / float(n_out - 1)


def draw_generator(shape: Sequence[int], output_size: Sequence[int]) -> tuple:
    """The random draws of ``RandomGenerator(output_size)`` for one slice of ``shape``, in the reference's order (dataset.py:156-159:
    ``random.random() > 0.5`` -> ``k = np.random.randint(0, 4)``, ``axis = np.random.randint(0, 2)``; else a SECOND
    ``random.random() > 0.5`` -> ``angle = np.random.randint(-20, 20)``; else nothing), turned into one ``icl_slice_augment``
    parameter record ``(n0, n1, branch, k, axis, M00, M01, M10, M11, off0, off1, z0, z1)``: five integers, eight doubles.
    ``M = [[cos, sin], [-sin, cos]]`` and ``off = centre - M @ centre`` are ``scipy.ndimage.rotate``'s own host expressions."""
    n0, n1 = (int(v) for v in shape)
    branch, k, axis = BRANCH_NONE, 0, 0
    m = (1.0, 0.0, 0.0, 1.0, 0.0, 0.0)
    if random.random() > 0.5:
        branch = BRANCH_ROTFLIP
        k = int(np.random.randint(0, 4))
        axis = int(np.random.randint(0, 2))
    elif random.random() > 0.5:
        branch = BRANCH_ROTATE
        m = rotate_matrix((n0, n1), int(np.random.randint(-20, 20)))
    r0, r1 = (n1, n0) if (branch == BRANCH_ROTFLIP and k & 1) else (n0, n1)      # rot90 swaps the extents for odd k
    return (n0, n1, branch, k, axis, *m, zoom_factor(r0, output_size[0]), zoom_factor(r1, output_size[1]))


def rotate_matrix(shape: Sequence[int], angle: int) -> tuple:
    """``(M00, M01, M10, M11, off0, off1)`` of ``scipy.ndimage.rotate(x, angle, reshape=False)`` for a 2-D ``x`` of ``shape``."""
    from scipy import special
    c, s = special.cosdg(angle), special.sindg(angle)
    mat = np.array([[c, s], [-s, c]])
    centre = (np.array([int(shape[0]), int(shape[1])], dtype=np.float64) - 1) / 2
    off = centre - mat @ centre
    return (float(mat[0, 0]), float(mat[0, 1]), float(mat[1, 0]), float(mat[1, 1]), float(off[0]), float(off[1]))


class DeviceSliceStore:
    """All slices of a split resident in HBM: ``images[i]`` fp32 [H, W], ``labels[i]`` uint8 [H, W]; extents free per slice."""

    def __init__(self, slices: Sequence[Tuple[np.ndarray, np.ndarray]], device):
        self.device = torch.device(device)
        self.images: List[torch.Tensor] = []
        self.labels: List[torch.Tensor] = []
        for image, label in slices:
            if image.shape != label.shape or image.ndim != 2:
                raise ValueError("a slice is an (image [H,W], label [H,W]) pair")
            self.images.append(torch.as_tensor(np.ascontiguousarray(image, dtype=np.float32)).to(self.device))
            self.labels.append(torch.as_tensor(np.ascontiguousarray(label, dtype=np.uint8)).to(self.device))

    @classmethod
    def from_dataset(cls, dataset: BaseDataSets, device):
        return cls([dataset.read_case(i) for i in range(len(dataset))], device)

    def __len__(self):
        return len(self.images)


class OnDeviceAugment2D:
    """``RandomGenerator(patch)`` + batch collation on the GPU: ``batch(indices)`` returns
    ``{'image': [B,1,O0,O1] fp32, 'label': [B,O0,O1] uint8}`` like the reference DataLoader's ``sampled_batch`` (without ``idx``:
    the caller holds the indices).  Parameters are drawn per sample in batch order unless ``params`` gives the records."""

    def __init__(self, store: DeviceSliceStore, patch_size: Sequence[int] = (256, 256)):
        self.store = store
        self.patch = tuple(int(v) for v in patch_size)
        if len(self.patch) != 2:
            raise ValueError("patch_size is (O0, O1)")

    def batch(self, indices: Sequence[int], params: Optional[Sequence[Sequence[float]]] = None):
        st = self.store
        n = len(indices)
        if params is None:
            params = [draw_generator(st.images[i].shape, self.patch) for i in indices]
        dev = st.device
        image = torch.empty((n, 1) + self.patch, dtype=torch.float32, device=dev)
        label = torch.empty((n,) + self.patch, dtype=torch.uint8, device=dev)
        L = _lib.lib()
        stream = _lib.stream_of(dev)
        for lo in range(0, n, SLICE_MAX_BATCH):
            chunk = list(indices[lo:lo + SLICE_MAX_BATCH])
            m = len(chunk)
            ptrs = ctypes.c_void_p * m
            ints = (ctypes.c_int32 * (5 * m))(*[int(v) for row in params[lo:lo + m] for v in row[:5]])
            dbls = (ctypes.c_double * (8 * m))(*[float(v) for row in params[lo:lo + m] for v in row[5:13]])
            _lib.check(L.icl_slice_augment(ptrs(*[st.images[i].data_ptr() for i in chunk]), ptrs(*[st.labels[i].data_ptr() for i in chunk]),
                                           ints, dbls, m, image[lo:].data_ptr(), label[lo:].data_ptr(), *self.patch, stream),
                       "slice_augment")
        return {"image": image, "label": label}


def resize_slices(src: torch.Tensor, output_size: Sequence[int]) -> torch.Tensor:
    """``scipy.ndimage.zoom(s, (O0 / H, O1 / W), order=0)`` of every slice of a contiguous ``[B, H, W]`` fp32 or int64 tensor with
    ONE launch (``icl_slice_resize``), scipy's zero last rows / columns included: both resizes of the 2-D validation loop."""
    if src.dim() != 3 or src.dtype not in (torch.float32, torch.int64):
        raise ValueError("resize_slices takes a [B, H, W] fp32 or int64 tensor")
    src = src.contiguous()
    b, n0, n1 = src.shape
    o0, o1 = (int(v) for v in output_size)
    zoom_factor(n0, o0), zoom_factor(n1, o1)             # the output extents are the ones scipy derives
    dst = torch.empty((b, o0, o1), dtype=src.dtype, device=src.device)
    _lib.check(_lib.lib().icl_slice_resize(src.data_ptr(), dst.data_ptr(), b, n0, n1, o0, o1, 0 if src.dtype == torch.float32 else 1,
                                           _lib.stream_of(src.device)), "slice_resize")
    return dst
