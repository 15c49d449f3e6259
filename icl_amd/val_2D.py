"""Slice-wise validation of the 2-D trainers — counterpart of the reference's ``val_2D.py``
(/root/reference/code/val_2D.py:10-54,109-131; called at train_inherent_consistent_unet_2D.py / ..._swinunet_2D.py).

``test_single_volume_ours(image, label, net, writer, iter_num, classes, patch_size)`` keeps the reference procedure — every slice
is resized to ``patch_size`` with ``scipy.ndimage.zoom(order=0)``, pushed through ``net(x, inference=True)``, arg-maxed and resized
back — but pushes ``slices_per_batch`` slices per forward (eval-mode networks are per-sample: BatchNorm uses its running statistics,
so batching does not change any slice's logits; the reference runs one slice per forward).  With the net on a HIP device the case goes
up once, both nearest-neighbour resizes are ONE launch each of the slice-resize kernel (``icl_slice_resize``: scipy's index mapping
bit for bit, the zero last rows / columns of its ``mode='constant'`` included) and the prediction never leaves the device;
``ICL_VAL_RESIZE=host`` (and every CPU net) keeps scipy on the host.  Metrics: Dice + HD95 with the reference's empty-mask conventions
(``icl_amd.val_3D.cal_metric``; HD95 parity unpinned — MedPy is not installed in the build image), scored for every class at once by
the metric kernels when the net is on a HIP device (``val_3D.cal_metric_multiclass``; ``ICL_VAL_METRICS=host``: numpy).
"""
from __future__ import annotations

import numpy as np
import torch
from scipy.ndimage import zoom

from .dataloaders.dataset import resize_slices
from .val_3D import _env_choice, _normalize_spacing, _postprocess_args, _score_prediction, cal_metric
from .val_3D import keep_components  # noqa: F401 — the filter of ``postprocess=``: reachable from here as before


def calculate_metric_percase(pred, gt, voxelspacing=None):
    """val_2D.py:10-22 (binarises its arguments like the reference): ``val_3D.cal_metric``, which takes the ground truth first and holds
    the empty-mask conventions.  ``voxelspacing``: HD95 in its units (``val_3D.binary_hd95``)."""
    return cal_metric(gt, pred, voxelspacing)


def val_resize_mode() -> str:
    """``ICL_VAL_RESIZE``: ``device`` (default) resizes the slices and the arg-max maps of a net on a HIP device with the slice-resize
    kernel, ``host`` forces scipy's ``zoom`` on the host (A/B runs).  CPU nets always take the host path."""
    return _env_choice("ICL_VAL_RESIZE", ("device", "host"))


def _zoom_gives(n_in, n_out):
    """scipy derives the output extent of ``zoom(x, n_out / n_in)`` as ``round(n_in * (n_out / n_in))``."""
    return n_in >= 1 and n_out >= 2 and int(round(n_in * (n_out / n_in))) == n_out


@torch.no_grad()
def _predict_volume(image, net, patch_size, inference_kw, slices_per_batch):
    """The prediction map [slices, H, W] int64: a numpy array from the host path, a device tensor from the device path."""
    dev = next(net.parameters()).device
    net.eval()
    n, x, y = image.shape
    p0, p1 = int(patch_size[0]), int(patch_size[1])
    if (dev.type == "cuda" and val_resize_mode() == "device" and n > 0 and image.dtype.kind in "fiu"
            and _zoom_gives(x, p0) and _zoom_gives(y, p1) and _zoom_gives(p0, x) and _zoom_gives(p1, y)):
        resized = resize_slices(torch.from_numpy(np.ascontiguousarray(image)).float().to(dev), (p0, p1))
        maps = torch.empty((n, p0, p1), dtype=torch.int64, device=dev)
        for lo in range(0, n, slices_per_batch):
            logits = net(resized[lo:lo + slices_per_batch].unsqueeze(1), **inference_kw)
            maps[lo:lo + logits.shape[0]] = torch.argmax(torch.softmax(logits, dim=1), dim=1)
        return resize_slices(maps, (x, y))
    prediction = np.zeros((n, x, y), dtype=np.int64)
    resized = np.stack([zoom(image[i], (patch_size[0] / x, patch_size[1] / y), order=0) for i in range(n)])
    for lo in range(0, n, slices_per_batch):
        batch = torch.from_numpy(resized[lo:lo + slices_per_batch]).unsqueeze(1).float().to(dev)
        out = torch.argmax(torch.softmax(net(batch, **inference_kw), dim=1), dim=1).cpu().numpy()
        for j in range(out.shape[0]):
            prediction[lo + j] = zoom(out[j], (x / patch_size[0], y / patch_size[1]), order=0)
    return prediction


def _score_volume(prediction, label, net, classes, voxelspacing=None, postprocess=None):
    """``[calculate_metric_percase(prediction == i, label == i) for i in 1..classes-1]`` of the stacked [slices, H, W] prediction (a numpy
    array or a device tensor), which goes through ``val_3D.keep_components`` as one 3-D map first when ``postprocess`` says so: the
    scoring step of ``val_3D`` (``_score_prediction``) — on the metric kernels with the net on a HIP device and a label map of the
    prediction's shape.  ``voxelspacing``: a number, or three for the [slices, H, W] volume — HD95 in its units."""
    if voxelspacing is not None:
        voxelspacing = _normalize_spacing(voxelspacing)
    return _score_prediction(prediction, label, classes, next(net.parameters()).device, voxelspacing, _postprocess_args(postprocess),
                             also=lambda gt, pred, _: gt.shape == pred.shape)


def test_single_volume_ours(image, label, net, writer=None, iter_num=0, classes=4, patch_size=(224, 224), slices_per_batch=16,
                            voxelspacing=None, postprocess=None):
    """val_2D.py:35-54: ``image`` / ``label`` are [1, slices, H, W] tensors (one case of the validation loader).  ``voxelspacing``: a
    number, or (slice thickness, pixel height, pixel width) — HD95 in its units; None: voxels, as the reference.  ``postprocess``: None (the
    reference), ``"largest"`` or a dict of ``val_3D.keep_components``' keywords — connected-component filter of the stacked prediction
    before it is scored."""
    _postprocess_args(postprocess)
    image = image.squeeze(0).cpu().detach().numpy()
    label = label.squeeze(0).cpu().detach().numpy()
    prediction = _predict_volume(image, net, patch_size, {"inference": True}, slices_per_batch)
    return _score_volume(prediction, label, net, classes, voxelspacing, postprocess)


def test_single_volume(image, label, net, classes, patch_size=(256, 256), slices_per_batch=16, voxelspacing=None, postprocess=None):
    """val_2D.py:109-131: the plain networks (``net(input)``).  ``voxelspacing`` and ``postprocess`` as in ``test_single_volume_ours``."""
    _postprocess_args(postprocess)
    image = image.squeeze(0).cpu().detach().numpy()
    label = label.squeeze(0).cpu().detach().numpy()
    prediction = _predict_volume(image, net, patch_size, {}, slices_per_batch)
    return _score_volume(prediction, label, net, classes, voxelspacing, postprocess)
