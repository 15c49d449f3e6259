"""Sliding-window validation on the device — counterpart of the reference's ``val_3D.py``
(/root/reference/code/val_3D.py:15-118).

``test_single_case_base`` keeps the reference's window grid (``ceil((dim - patch) / stride) + 1`` positions per axis, the
last one clamped to ``dim - patch``, zero padding of small volumes :18-41,43-55) but keeps the volume, the score map and
the count map in HBM and pushes several windows per forward (the backbone is per-sample, so batching windows does not
change any window's logits); the reference moves every window host->device->host and accumulates in numpy (:57-73).
``cal_metric`` reproduces the empty-mask conventions (:85-97).  Dice is computed here; HD95 follows MedPy 0.4.0's
published definition (``medpy.metric.binary.hd95``: 95th percentile of the symmetric surface distances, surfaces from a
connectivity-1 erosion, distances from ``scipy.ndimage.distance_transform_edt``) — MedPy itself is not installed in the
build image, so the HD95 half is "parity unpinned" (DESIGN.md §2).

On a HIP device the stretch between the volume and the label map — window gather, soft-max, accumulation of the score and weight
maps, division, arg-max, crop — runs on the window kernels (csrc/kernels/window.h, ``ops.window_*``) in both loops;
``ICL_VAL_WINDOWS=aten`` keeps the ATen loops, which also serve host tensors.  ``mode="gaussian"`` blends overlapping windows with a
Gaussian importance map on either path.  ``mirror_axes=`` turns mirror test-time augmentation on in both loops: every window is predicted
once per subset of those axes, mirrored, and each prediction is mirrored back into the average — in the indexing of the same kernels, at
one forward per pass and no further tensor.
"""
from __future__ import annotations

import math
import os

import numpy as np
import torch


def _env_choice(name, allowed):
    """The environment variable ``name``: one of the two words ``allowed``, the first when it is not set; anything else is a ValueError."""
    mode = os.environ.get(name, allowed[0])
    if mode not in allowed:
        raise ValueError(f"{name} must be {allowed[0]!r} or {allowed[1]!r}, got {mode!r}")
    return mode


def val_windows_mode() -> str:
    """``ICL_VAL_WINDOWS``: ``device`` (default) runs the sliding window of both 3-D validation loops — window gather, soft-max and
    accumulation, division, arg-max and crop — on the window kernels (csrc/kernels/window.h) when the volume is an fp32 tensor on a HIP
    device; ``aten`` forces the ATen loop (A/B runs).  Host tensors and other dtypes always take the ATen loop."""
    return _env_choice("ICL_VAL_WINDOWS", ("device", "aten"))


_WINDOW_MAX_CLASSES = 256      # icl_window_accumulate / icl_window_finalize
_WINDOW_MAX_BATCH = 16         # windows per launch


def gaussian_importance_map(roi_size, sigma_scale=0.125) -> torch.Tensor:
    """The window weights of ``mode="gaussian"``, fp32 [r0, r1, r2] on the host.  Built in float64, per axis: with c = r // 2 and
    sigma = sigma_scale * r the factor is g(i) = exp(-(i - c)^2 / (2 sigma^2)); the map is the product of the three factors, divided by
    its maximum, cast to fp32 and floored at 1e-3.  This FOLLOWS MONAI's Gaussian mode (``compute_importance_map``), which filters a delta
    at the centre with an erf-integrated Gaussian kernel of the same sigma and floors the result likewise; MONAI is not installed in the build
    image, so parity with its map is unpinned, like the window grid."""
    roi = [int(r) for r in roi_size]
    scales = [float(sigma_scale)] * len(roi) if np.isscalar(sigma_scale) else [float(v) for v in sigma_scale]
    if len(scales) != len(roi):
        raise ValueError(f"sigma_scale needs one value or {len(roi)}, got {sigma_scale!r}")
    m = np.ones((), dtype=np.float64)
    for r, sc in zip(roi, scales):
        i = np.arange(r, dtype=np.float64)
        sigma = sc * r
        m = m[..., None] * np.exp(-((i - (r // 2)) ** 2) / (2.0 * sigma * sigma))
    m = m / m.max()
    return torch.from_numpy(m.astype(np.float32)).clamp_(min=1e-3)


def _importance_map(mode, roi_size, sigma_scale, device):
    """None for ``constant``, the Gaussian map on ``device`` for ``gaussian``; any other mode is a ValueError."""
    if mode == "constant":
        return None
    if mode == "gaussian":
        return gaussian_importance_map(roi_size, sigma_scale).to(device)
    raise ValueError(f"sliding-window mode must be 'constant' or 'gaussian', got {mode!r}")


def _mirror_masks(mirror_axes):
    """``mirror_axes=`` of the validation loops -> the mirror masks of test-time augmentation, or None.  ``mirror_axes``: None (no
    augmentation) or a sequence of distinct axes out of 0, 1, 2 — the window's three spatial axes — which may be empty; anything else is
    a ValueError.  A mask is a subset of those axes as an integer, bit a set for axis a; all 2^len(mirror_axes) of them, in increasing
    order, so mask 0 (the window as it is) comes first."""
    if mirror_axes is None:
        return None
    try:
        axes = None if isinstance(mirror_axes, (str, bytes)) else list(mirror_axes)
    except TypeError:
        axes = None
    if (axes is None or any(isinstance(a, bool) or not isinstance(a, (int, np.integer)) or a not in (0, 1, 2) for a in axes)
            or len(set(axes)) != len(axes)):
        raise ValueError(f"mirror_axes must be None or distinct axes out of 0, 1, 2, got {mirror_axes!r}")
    masks = [0]
    for a in sorted(int(a) for a in axes):
        masks += [m | (1 << a) for m in masks]
    return masks


def _mask_dims(mask, first):
    """The tensor axes of a mirror mask where the window's spatial axes start at ``first``."""
    return [first + a for a in range(3) if (mask >> a) & 1]


def _window_kernels_apply(t, num_classes=1) -> bool:
    return (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and 1 <= num_classes <= _WINDOW_MAX_CLASSES
            and val_windows_mode() == "device")


@torch.no_grad()
def test_single_case_base(net, net_type, image, stride_xy, stride_z, patch_size, num_classes=1, windows_per_batch=4,
                          return_score=False, mode="constant", mirror_axes=None):
    """image: numpy [W,H,D] (the reference's h5 layout), or channel-first [C,W,H,D] for a multi-modal net.  Returns the label map
    (numpy int64 [W,H,D]).  ``mode``: ``constant`` (the
    reference's plain average over overlapping windows) or ``gaussian`` (``gaussian_importance_map`` at sigma_scale 0.125).
    ``mirror_axes``: None, or the axes out of 0, 1, 2 (W, H, D) of mirror test-time augmentation (``_run_windows``); ``windows_per_batch``
    then counts passes."""
    label_map, score = _single_case_on_device(net, net_type, image, stride_xy, stride_z, patch_size, num_classes, windows_per_batch, mode,
                                              return_score, mirror_axes)
    if return_score:
        return label_map.cpu().numpy(), score.cpu().numpy()
    return label_map.cpu().numpy()


def _fits_brats(num_classes, roi):
    """When the BraTS loop stays on the window kernels: fp32 logits of exactly [n, num_classes, *roi]."""
    roi = tuple(int(r) for r in roi)
    return lambda pred, n: tuple(pred.shape) == (n, num_classes, *roi) and pred.dtype == torch.float32


def _fits_amos(roi, device):
    """When the AMOS loop stays on the window kernels: a tensor [n, 1 <= C <= 256, *roi] of any dtype on ``device`` (the loop casts it)."""
    return lambda pred, n: (torch.is_tensor(pred) and pred.dim() == 5 and pred.shape[0] == n and list(pred.shape[2:]) == list(roi)
                            and 1 <= pred.shape[1] <= _WINDOW_MAX_CLASSES and pred.device == device)


def _run_windows(vols, roi, pads, psize, starts, per_forward, forward, imp, softmax, want, kernels, fits, num_classes=None, masks=None):
    """The sliding window of both validation loops, and the only place that walks window origins.  ``vols`` fp32 [B, Cin, s0, s1, s2],
    unpadded; ``pads`` the (before, after) zero padding per axis that brings it to the extent ``psize``; ``starts`` the windows as (batch
    index, o0, o1, o2) in the padded frame, in loop order, ``per_forward`` of them per ``forward(win)`` (win [n, Cin, *roi]); ``imp`` the
    importance map [*roi] or None.  A window adds ``softmax(pred, 1)`` (``softmax``) or ``pred.float()`` to the score map — times ``imp``
    when there is one — and 1, or ``imp``, to the weight map; then come score / weight, the arg-max over the classes and the crop to the
    volume.  ``want``: ``"label"``, ``"quotients"`` or ``"both"``.  Returns ((label maps int64 [B, *size] or None, quotients fp32
    [B, C, *size] or None), handed).

    ``kernels``: gather, accumulate and finalize on the window kernels (``ops.window_*``: a launch takes at most 16 windows, all of one
    volume; the gather zero-fills, so the volume is not padded), else in ATen — the same adds in the same order.  The kernel form gives
    up when ``fits(pred, n)``, the caller's rule, is false for the prediction of the FIRST batch: the loop goes on in ATen with that
    prediction — ``handed``, None when there was no hand-over — so ``forward`` sees every batch once.  ``num_classes``: the channels of the score map; None takes them from the first prediction.  The kernel form
    computes only what is wanted (quotients alone where nothing is cropped: divided in place); the ATen form has the quotients anyway
    and returns them whatever ``want`` says.

    ``masks`` (``_mirror_masks``; None: none of this) — mirror test-time augmentation.  The loop walks PASSES instead of windows: a pass is
    a (window, mask) pair, window-major and mask-minor, and ``per_forward`` and the 16 of a launch count passes.  A pass with mask f
    predicts ``flip(win, axes of f)`` and adds ``flip(value, the same axes)`` — times ``imp``, which is NOT flipped: it is indexed in the
    volume's frame — so the quotient is the mean over all passes covering a voxel.  The kernel form does both flips in the indexing of
    the gather and of the accumulate (``flips=``), the ATen form with ``torch.flip``; the hand-over works on passes as it does on
    windows."""
    from . import ops
    b, cin = vols.shape[:2]
    size, roi, psize = tuple(vols.shape[2:]), tuple(int(r) for r in roi), tuple(psize)
    a = tuple(p[0] for p in pads)
    r0, r1, r2 = roi

    def padded(v):
        return torch.nn.functional.pad(v, [n for p, q in reversed(pads) for n in (p, q)]) if any(p + q for p, q in pads) else v
    vols = vols.contiguous() if kernels else padded(vols)
    score = weight = handed = None
    if masks is not None:
        starts = [s + (f,) for s in starts for f in masks]

    def flips(run):
        return None if masks is None else [c[4] for c in run]
    for i in range(0, len(starts), per_forward):
        chunk = starts[i:i + per_forward]
        if kernels:
            runs, k = [], 0      # runs of windows of one volume, at most 16 each: one launch per run
            while k < len(chunk):
                e = k + 1
                while e < len(chunk) and e - k < _WINDOW_MAX_BATCH and chunk[e][0] == chunk[k][0]:
                    e += 1
                runs.append((k, e))
                k = e
            win = torch.empty((len(chunk), cin, *roi), dtype=torch.float32, device=vols.device)
            for k, e in runs:
                ops.window_gather(vols[chunk[k][0]], [c[1:4] for c in chunk[k:e]], roi, a, psize, out=win[k:e], flips=flips(chunk[k:e]))
        else:
            wins = [vols[bi, :, z:z + r0, y:y + r1, x:x + r2] for bi, z, y, x, *_ in chunk]
            if masks is not None:
                wins = [w.flip(_mask_dims(c[4], 1)) if c[4] else w for w, c in zip(wins, chunk)]
            win = torch.stack(wins).contiguous()
        pred = forward(win)
        if score is None:
            if kernels and not fits(pred, len(chunk)):      # hand-over: this batch has been through the network
                kernels, handed, vols = False, pred, padded(vols)
            nc = pred.shape[1] if num_classes is None else num_classes
            score = torch.zeros((b, nc, *psize), dtype=torch.float32, device=vols.device)
            weight = torch.zeros((b, *psize), dtype=torch.float32, device=vols.device)
        if kernels:
            pred = pred.float()
            for k, e in runs:
                bi = chunk[k][0]
                ops.window_accumulate(pred[k:e], [c[1:4] for c in chunk[k:e]], score[bi], weight[bi], imp, softmax=softmax,
                                      flips=flips(chunk[k:e]))
            continue
        if softmax:
            pred = torch.softmax(pred, dim=1)
        for j, (bi, z, y, x, *f) in enumerate(chunk):
            value = pred[j] if softmax else pred[j].float()
            if f and f[0]:
                value = value.flip(_mask_dims(f[0], 1))
            if imp is None:
                score[bi, :, z:z + r0, y:y + r1, x:x + r2] += value
                weight[bi, z:z + r0, y:y + r1, x:x + r2] += 1
            else:
                score[bi, :, z:z + r0, y:y + r1, x:x + r2] += value * imp
                weight[bi, z:z + r0, y:y + r1, x:x + r2] += imp
    if kernels:
        labels, quots = [], []
        for bi in range(b):
            res = ops.window_finalize(score[bi], weight[bi], a, size, return_score=want != "label", label=want != "quotients")
            lab, quot = res if want == "both" else (res, None) if want == "label" else (None, res)
            labels.append(lab)
            quots.append(quot)

        def join(ts):
            return None if ts[0] is None else ts[0].unsqueeze(0) if b == 1 else torch.stack(ts)
        return (join(labels), join(quots)), handed
    score = score / weight.unsqueeze(1)
    crop = tuple(slice(p, p + n) for p, n in zip(a, size))
    label = torch.argmax(score, dim=1)[(slice(None),) + crop] if want != "quotients" else None
    return (label, score[(slice(None), slice(None)) + crop]), handed


@torch.no_grad()
def _single_case_on_device(net, net_type, image, stride_xy, stride_z, patch_size, num_classes=1, windows_per_batch=4, mode="constant",
                           want_score=True, mirror_axes=None):
    """``test_single_case_base`` up to the copy to the host: (label map int64 [W,H,D], score [C,W,H,D]) on the net's device.  On a HIP
    device the windows are gathered, soft-maxed, accumulated, divided and arg-maxed by the window kernels (``ICL_VAL_WINDOWS``; the score
    is None when ``want_score`` is false — the kernel then writes the label map alone); elsewhere, and when the network's output is not
    fp32 [n, num_classes, *patch_size], in ATen (``_run_windows``).  Both walk the same window grid — with ``mirror_axes``, the same passes of mirror test-time augmentation.
    ``image``: [W,H,D], or channel-first [C,W,H,D] for a multi-modal net (``in_channels = C``): pads and window grid come from the last
    three extents, and the windows the net sees are [n, C, *patch_size]."""
    masks = _mirror_masks(mirror_axes)
    dev = next(net.parameters()).device
    if image.ndim not in (3, 4):
        raise ValueError(f"a case is an image [W,H,D] or [C,W,H,D], got shape {tuple(image.shape)}")
    extents = tuple(image.shape[-3:])
    pads = []
    for dim, p in zip(extents, patch_size):
        tot = max(p - dim, 0)
        pads.append((tot // 2, tot - tot // 2))
    vol = torch.as_tensor(np.ascontiguousarray(image), dtype=torch.float32, device=dev)
    imp = _importance_map(mode, patch_size, 0.125, dev)
    ww, hh, dd = (n + a + b for n, (a, b) in zip(extents, pads))          # the padded extents
    sx = math.ceil((ww - patch_size[0]) / stride_xy) + 1
    sy = math.ceil((hh - patch_size[1]) / stride_xy) + 1
    sz = math.ceil((dd - patch_size[2]) / stride_z) + 1
    starts = []
    for x in range(sx):
        xs = min(stride_xy * x, ww - patch_size[0])
        for y in range(sy):
            ys = min(stride_xy * y, hh - patch_size[1])
            for z in range(sz):
                zs = min(stride_z * z, dd - patch_size[2])
                starts.append((0, xs, ys, zs))
    icl = net_type in ("swinunetr_icl", "unet_3D_icl")
    (label_map, score), _ = _run_windows(
        vol[None] if vol.ndim == 4 else vol[None, None], patch_size, pads, (ww, hh, dd), starts, windows_per_batch,
        lambda win: net(win, inference=True) if icl else net(win),
        imp, True, "both" if want_score else "label", _window_kernels_apply(vol, num_classes), _fits_brats(num_classes, patch_size), num_classes, masks)
    return label_map[0], None if score is None else score[0]


def binary_dice(pred, gt) -> float:
    """medpy.metric.binary.dc: 2|A&B| / (|A|+|B|) (0 when both are empty)."""
    pred = np.asarray(pred).astype(bool)
    gt = np.asarray(gt).astype(bool)
    inter = np.count_nonzero(pred & gt)
    size = np.count_nonzero(pred) + np.count_nonzero(gt)
    return 2.0 * inter / float(size) if size else 0.0


def _normalize_spacing(voxelspacing):
    """A voxel spacing as three floats: a scalar is broadcast (scipy's ``_normalize_sequence``), a sequence needs three entries; every
    entry finite and positive.  Anything else is a ValueError — on the device path and on the numpy path alike."""
    if isinstance(voxelspacing, (str, bytes)):
        raise ValueError(f"voxelspacing must be a number or three numbers, got {voxelspacing!r}")
    if torch.is_tensor(voxelspacing):
        voxelspacing = voxelspacing.tolist()
    try:
        sp = [float(v) for v in voxelspacing] if np.ndim(voxelspacing) else [float(voxelspacing)] * 3
    except (TypeError, ValueError):
        raise ValueError(f"voxelspacing must be a number or three numbers, got {voxelspacing!r}") from None
    if len(sp) != 3 or np.ndim(voxelspacing) > 1:
        raise ValueError(f"voxelspacing must be a number or three numbers, got {voxelspacing!r}")
    if not all(math.isfinite(v) and v > 0 for v in sp):
        raise ValueError(f"voxelspacing must be finite and positive, got {voxelspacing!r}")
    return tuple(sp)


def _normalize_tolerance(tolerance) -> float:
    tol = float(tolerance)
    if not (math.isfinite(tol) and tol >= 0):
        raise ValueError(f"tolerance must be finite and not negative, got {tolerance!r}")
    return tol


def _sampling_for(shape, voxelspacing):
    """scipy's ``sampling`` for a map of this shape: the three entries apply to the last three axes; leading axes must have length 1 (the
    AMOS loop scores [1, D, H, W] maps) and get spacing 1 — no distance runs along them."""
    sp = _normalize_spacing(voxelspacing)
    if len(shape) < 3 or any(n != 1 for n in shape[:-3]):
        raise ValueError(f"voxelspacing needs a 3-D map (leading axes of length 1 allowed), got shape {tuple(shape)}")
    return (1.0,) * (len(shape) - 3) + sp


def _surface_distances(result, reference, voxelspacing=None):
    """MedPy 0.4.0's ``__surface_distances`` (connectivity 1): the distances of the border voxels of ``result`` to the border of
    ``reference``, with ``sampling=voxelspacing`` in the distance transform when a spacing is given."""
    from scipy.ndimage import binary_erosion, distance_transform_edt, generate_binary_structure
    result = np.atleast_1d(result.astype(bool))
    reference = np.atleast_1d(reference.astype(bool))
    fp = generate_binary_structure(result.ndim, 1)
    rb = result ^ binary_erosion(result, structure=fp, iterations=1)
    fb = reference ^ binary_erosion(reference, structure=fp, iterations=1)
    if voxelspacing is None:
        dt = distance_transform_edt(~fb)
    else:
        dt = distance_transform_edt(~fb, sampling=_sampling_for(result.shape, voxelspacing))
    return dt[rb]


def binary_hd95(pred, gt, voxelspacing=None) -> float:
    """medpy.metric.binary.hd95 (MedPy 0.4.0): 95th percentile of both directed surface-distance sets, in the units of ``voxelspacing``
    (voxels when None)."""
    a = _surface_distances(np.asarray(pred), np.asarray(gt), voxelspacing)
    b = _surface_distances(np.asarray(gt), np.asarray(pred), voxelspacing)
    return float(np.percentile(np.hstack((a, b)), 95))


def binary_hd(pred, gt, voxelspacing=None) -> float:
    """medpy.metric.binary.hd: the larger of the two directed maxima of the surface distances."""
    a = _surface_distances(np.asarray(pred), np.asarray(gt), voxelspacing)
    b = _surface_distances(np.asarray(gt), np.asarray(pred), voxelspacing)
    return float(max(a.max(), b.max()))


def binary_asd(result, reference, voxelspacing=None) -> float:
    """medpy.metric.binary.asd: the mean distance of the border voxels of ``result`` to the border of ``reference`` (directed)."""
    return float(_surface_distances(np.asarray(result), np.asarray(reference), voxelspacing).mean())


def binary_assd(pred, gt, voxelspacing=None) -> float:
    """medpy.metric.binary.assd: the mean of the two directed average surface distances."""
    return float(np.mean((binary_asd(pred, gt, voxelspacing), binary_asd(gt, pred, voxelspacing))))


def binary_nsd(pred, gt, tolerance, voxelspacing=None) -> float:
    """Normalised surface distance (surface Dice) at ``tolerance`` on the voxel borders used everywhere else here:
    (#{p in dP: d(p, dG) <= tau} + #{g in dG: d(g, dP) <= tau}) / (|dP| + |dG|).  This is the VOXEL-BORDER NSD: every border voxel
    counts once.  It is not the surface-area-weighted NSD of DeepMind's ``surface-distance`` package, which weights surface elements
    by their area and which challenge rankings may use; the two agree in the limit of fine grids, not voxel for voxel."""
    tol = _normalize_tolerance(tolerance)
    a = _surface_distances(np.asarray(pred), np.asarray(gt), voxelspacing)
    b = _surface_distances(np.asarray(gt), np.asarray(pred), voxelspacing)
    return float((np.count_nonzero(a <= tol) + np.count_nonzero(b <= tol)) / (len(a) + len(b)))


def cal_metric(gt, pred, voxelspacing=None):
    """val_3D.py:85-97, including the hard-coded fall-backs for empty masks.  ``voxelspacing`` (a number or three): HD95 in its units."""
    pred = np.asarray(pred) > 0
    gt = np.asarray(gt) > 0
    if voxelspacing is not None:
        voxelspacing = _normalize_spacing(voxelspacing)
    if pred.sum() > 0 and gt.sum() > 0:
        if voxelspacing is None:
            return binary_dice(pred, gt), binary_hd95(pred, gt)
        return binary_dice(pred, gt), binary_hd95(pred, gt, voxelspacing)
    if pred.sum() > 0 and gt.sum() == 0:
        return 0, 373.128664
    if pred.sum() == 0 and gt.sum() > 0:
        return 0, 373.128664
    return 1, 0


# --------------------------------------------------------------------------------------------------------------------
# All foreground classes at once on the device (kernels/metrics.h, include/icl_hip.h icl_seg_metrics)
# --------------------------------------------------------------------------------------------------------------------

def val_metrics_mode() -> str:
    """``ICL_VAL_METRICS``: ``device`` (default) scores label maps that are on a HIP device with the metric kernels, ``host`` forces the
    numpy path of ``cal_metric`` (A/B runs).  Host data always take the numpy path."""
    return _env_choice("ICL_VAL_METRICS", ("device", "host"))


def hd95_from_order_stats(n: int, sq0, sq1) -> float:
    """``np.percentile(x, 95)`` of n >= 2 distances given the SQUARED distances at ranks k0 = floor(0.95 (n - 1)) and k0 + 1 of the sorted
    set — numpy's ``linear`` method step for step (virtual index (n - 1) * 0.95, gamma its fractional part, ``_lerp``) in float64.
    sqrt of an exact integer is correctly rounded, so this is bit-equal to the percentile of the distance transform's values (the
    integer path); the floating path passes its squares as floats, exact whenever the distance transform's sums are)."""
    v = (n - 1) * np.true_divide(95, 100)
    gamma = v - np.floor(v)
    a, b = np.sqrt(np.float64(sq0)), np.sqrt(np.float64(sq1))
    diff = b - a
    return float(b - diff * (1 - gamma) if gamma >= 0.5 else a + diff * gamma)


def _metric_from_record(rec):
    """One row of ``ops.seg_metrics`` -> what ``cal_metric`` returns for that class (values and types)."""
    np_, ng, inter, n, sq0, sq1 = (int(v) for v in rec)
    if np_ > 0 and ng > 0:
        return 2.0 * inter / float(np_ + ng), hd95_from_order_stats(n, sq0, sq1)
    if np_ > 0 or ng > 0:
        return 0, 373.128664
    return 1, 0


def _cal_metric_kernels(gt, pred, num_classes):
    from . import ops
    return [_metric_from_record(r) for r in ops.seg_metrics(pred, gt, num_classes).cpu().tolist()]


def _device_metrics_apply(gt, pred, num_classes) -> bool:
    from . import ops
    return (torch.is_tensor(gt) and torch.is_tensor(pred) and gt.is_cuda and pred.is_cuda and val_metrics_mode() == "device"
            and 2 <= num_classes <= 256
            and gt.shape == pred.shape and gt.dtype in ops._SEG_DTYPES and pred.dtype in ops._SEG_DTYPES
            and ops.seg_metrics_shape(pred) is not None)


def cal_metric_multiclass(gt, pred, num_classes, voxelspacing=None):
    """``[cal_metric(gt == c, pred == c) for c in 1..num_classes-1]`` with identical values and types.  Label maps on a HIP device
    (uint8 / bool or int64; 3-D, or with leading axes of length 1) are scored by the metric kernels and stay there — six
    integers per class come back; anything else (and num_classes outside 2..256) takes the numpy path unchanged
    (``ICL_VAL_METRICS=host`` forces it).  ``voxelspacing`` (a number, or three: the voxel size along the last three axes) gives HD95 in its
    units: any spacing, all ones included, takes the floating-point surface kernels (kernels/metrics_surface.h) for 3-D maps on a HIP
    device and ``cal_metric(..., voxelspacing)`` elsewhere; None is the integer path above, untouched."""
    if voxelspacing is not None:
        sp = _normalize_spacing(voxelspacing)
        if _device_surface_apply(gt, pred, num_classes):
            return _cal_metric_surface_kernels(gt, pred, num_classes, sp)
        gt, pred = _to_host(gt), _to_host(pred)
        return [cal_metric(gt == c, pred == c, sp) for c in range(1, num_classes)]
    if _device_metrics_apply(gt, pred, num_classes):
        return _cal_metric_kernels(gt, pred, num_classes)
    if torch.is_tensor(gt) and gt.is_cuda:
        gt = gt.cpu().numpy()
    if torch.is_tensor(pred) and pred.is_cuda:
        pred = pred.cpu().numpy()
    return [cal_metric(gt == c, pred == c) for c in range(1, num_classes)]


# --------------------------------------------------------------------------------------------------------------------
# Surface metrics in the spacing's units (kernels/metrics_surface.h, include/icl_hip.h icl_seg_surface_metrics)
# --------------------------------------------------------------------------------------------------------------------

_EMPTY_DISTANCE = 373.128664      # the reference's value for a class present in only one of the maps (val_3D.py:85-97)
SURFACE_METRIC_KEYS = ("dice", "hd95", "hd", "assd", "asd_pred_gt", "asd_gt_pred", "nsd")


def _to_host(t):
    return t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def _device_surface_apply(gt, pred, num_classes) -> bool:
    """The floating-point kernels take exactly 3-D maps (a leading axis of length 1 makes every voxel a border voxel under the N-D
    erosion, which only the integer entry point knows): anything else goes to the numpy path."""
    return _device_metrics_apply(gt, pred, num_classes) and gt.dim() == 3


def _surface_empty_record(n_pred, n_gt):
    """The reference's empty-mask conventions, extended: both empty — dice 1, distances 0, nsd 1.0; exactly one empty — dice 0, every
    distance 373.128664, nsd 0.0.  Dice and the distances keep the reference's types (ints 1 / 0 / 0, the float constant)."""
    if n_pred > 0 or n_gt > 0:
        rec = {k: _EMPTY_DISTANCE for k in SURFACE_METRIC_KEYS}
        rec["dice"], rec["nsd"] = 0, 0.0
    else:
        rec = {k: 0 for k in SURFACE_METRIC_KEYS}
        rec["dice"], rec["nsd"] = 1, 1.0
    return rec


def _surface_metrics_host(pred, gt, voxelspacing=None, tolerance=1.0):
    """All seven quantities of one class on the host (numpy / scipy): the two directed distance sets are formed once."""
    pred = np.asarray(pred) > 0
    gt = np.asarray(gt) > 0
    tol = _normalize_tolerance(tolerance)
    if voxelspacing is not None:
        voxelspacing = _normalize_spacing(voxelspacing)
    n_pred, n_gt = int(pred.sum()), int(gt.sum())
    if n_pred == 0 or n_gt == 0:
        return _surface_empty_record(n_pred, n_gt)
    a = _surface_distances(pred, gt, voxelspacing)
    b = _surface_distances(gt, pred, voxelspacing)
    apg, agp = float(a.mean()), float(b.mean())
    return {"dice": binary_dice(pred, gt), "hd95": float(np.percentile(np.hstack((a, b)), 95)), "hd": float(max(a.max(), b.max())),
            "assd": float(np.mean((apg, agp))), "asd_pred_gt": apg, "asd_gt_pred": agp,
            "nsd": float((np.count_nonzero(a <= tol) + np.count_nonzero(b <= tol)) / (len(a) + len(b)))}


def _surface_from_record(cnt, val):
    """One row of ``ops.seg_surface_metrics`` -> the dict of ``surface_metrics_multiclass`` for that class."""
    n_pred, n_gt, inter, bp, bg, wp, wg = (int(v) for v in cnt)
    if n_pred == 0 or n_gt == 0:
        return _surface_empty_record(n_pred, n_gt)
    sq0, sq1, mx0, mx1, sum0, sum1 = (np.float64(v) for v in val)
    apg, agp = float(sum0 / bp), float(sum1 / bg)
    return {"dice": 2.0 * inter / float(n_pred + n_gt), "hd95": hd95_from_order_stats(bp + bg, sq0, sq1),
            "hd": float(max(np.sqrt(mx0), np.sqrt(mx1))), "assd": float(np.mean((apg, agp))), "asd_pred_gt": apg, "asd_gt_pred": agp,
            "nsd": float((wp + wg) / (bp + bg))}


def _surface_records_kernels(gt, pred, num_classes, spacing, tolerance):
    from . import ops
    counts, values = ops.seg_surface_metrics(pred, gt, num_classes, spacing, tolerance)
    return [_surface_from_record(c, v) for c, v in zip(counts.cpu().tolist(), values.cpu().tolist())]


def _cal_metric_surface_kernels(gt, pred, num_classes, spacing):
    """``cal_metric``'s pairs (values and types) from the floating-point kernels."""
    out = []
    for rec in _surface_records_kernels(gt, pred, num_classes, spacing, 1.0):
        out.append((rec["dice"], rec["hd95"]))
    return out


def surface_metrics_multiclass(gt, pred, num_classes, voxelspacing=None, tolerance=1.0):
    """Per foreground class c in 1..num_classes-1 a dict {dice, hd95, hd, assd, asd_pred_gt, asd_gt_pred, nsd} of ``gt == c`` against
    ``pred == c``: MedPy 0.4.0's ``dc``, ``hd95``, ``hd``, ``assd``, ``asd(pred, gt)``, ``asd(gt, pred)`` with ``voxelspacing`` (a number or three;
    None: unit spacing) and the voxel-border NSD at ``tolerance`` (``binary_nsd``), distances in the spacing's units.  3-D label maps on a HIP
    device are scored by the surface kernels (kernels/metrics_surface.h) under the rule of ``cal_metric_multiclass``; anything else, and
    ``ICL_VAL_METRICS=host``, by numpy.  Empty masks extend the reference's conventions: both empty — dice 1, distances 0, nsd 1.0; exactly one
    empty — dice 0, every distance 373.128664, nsd 0.0."""
    sp = _normalize_spacing(1.0 if voxelspacing is None else voxelspacing)
    tol = _normalize_tolerance(tolerance)
    if _device_surface_apply(gt, pred, num_classes):
        return _surface_records_kernels(gt, pred, num_classes, sp, tol)
    gt, pred = _to_host(gt), _to_host(pred)
    return [_surface_metrics_host(pred == c, gt == c, sp, tol) for c in range(1, num_classes)]


# --------------------------------------------------------------------------------------------------------------------
# Connected-component post-processing between the arg-max and the scores (kernels/components.h, include/icl_hip.h icl_seg_components)
# --------------------------------------------------------------------------------------------------------------------

def components_mode() -> str:
    """``ICL_VAL_COMPONENTS``: ``device`` (default) filters label maps that are on a HIP device with the component kernels, ``host`` forces
    the scipy path (A/B runs).  Host data always take scipy."""
    return _env_choice("ICL_VAL_COMPONENTS", ("device", "host"))


def _components_args(num_classes, connectivity, keep_largest, min_size):
    if isinstance(num_classes, bool) or not isinstance(num_classes, (int, np.integer)) or num_classes < 2:
        raise ValueError(f"num_classes must be an integer >= 2, got {num_classes!r}")
    if isinstance(connectivity, bool) or not isinstance(connectivity, (int, np.integer)) or connectivity not in (1, 2, 3):
        raise ValueError(f"connectivity must be 1, 2 or 3, got {connectivity!r}")
    if isinstance(min_size, bool) or not isinstance(min_size, (int, np.integer)) or min_size < 0:
        raise ValueError(f"min_size must be an integer >= 0, got {min_size!r}")
    return int(num_classes), int(connectivity), bool(keep_largest), int(min_size)


def _keep_components_host(m3, num_classes, connectivity, keep_largest, min_size):
    """The filter on a 3-D numpy map, restated on ``scipy.ndimage.label`` (one labelling per class): int64 map of the kept voxels' classes.
    scipy numbers the components in raster order of their first voxel, so ``np.argmax`` over their sizes is the largest, and among equal
    sizes the one that starts first — the kernels' tie rule."""
    from scipy.ndimage import generate_binary_structure, label
    structure = generate_binary_structure(3, connectivity)
    out = np.zeros(m3.shape, dtype=np.int64)
    for c in range(1, num_classes):
        lab, n = label(m3 == c, structure)
        if n == 0:
            continue
        sizes = np.bincount(lab.ravel(), minlength=n + 1)
        sizes[0] = 0
        keep = sizes >= min_size
        if keep_largest:
            largest = np.zeros_like(keep)
            largest[int(np.argmax(sizes))] = True
            keep &= largest
        keep[0] = False
        out[keep[lab]] = c
    return out


def keep_components(label_map, num_classes, connectivity=1, keep_largest=True, min_size=0):
    """Connected-component post-processing of a label map: per class c in 1..num_classes-1 the components of ``label_map == c``
    (``connectivity`` 1 / 2 / 3: 6 / 18 / 26 neighbours) that are kept stay, every other voxel becomes 0.  A component is kept iff (not
    ``keep_largest`` or it is its class's largest; among equal sizes the one whose first voxel comes first in raster order) and it has at
    least ``min_size`` voxels.  Labels outside 1..num_classes-1 are background.  The map is 3-D, or 3-D behind leading axes of length 1 (they
    are squeezed first: such an axis adds no neighbour).  Returns what it was given — a tensor on the same device or a numpy array, same
    dtype and shape.  A uint8 / bool / int64 tensor on a HIP device is filtered by the component kernels and stays there
    (``ICL_VAL_COMPONENTS=host`` forces scipy); anything else by scipy on the host."""
    nc, k, largest, ms = _components_args(num_classes, connectivity, keep_largest, min_size)
    shape = tuple(label_map.shape)
    if len(shape) < 3 or any(s != 1 for s in shape[:-3]):
        raise ValueError(f"keep_components needs a 3-D label map (leading axes of length 1 allowed), got shape {shape}")
    if torch.is_tensor(label_map):
        from . import ops
        if (label_map.is_cuda and components_mode() == "device" and nc <= 256 and label_map.dtype in ops._SEG_DTYPES
                and 0 < label_map.numel() < 2 ** 31 - 1):
            return ops.seg_filter_components(label_map, nc, k, largest, ms)
        host = label_map.cpu().numpy()
        out = _keep_components_host(host.reshape(shape[-3:]), nc, k, largest, ms)
        return torch.from_numpy(out.reshape(shape).astype(host.dtype)).to(label_map.device)
    host = np.asarray(label_map)
    return _keep_components_host(host.reshape(shape[-3:]), nc, k, largest, ms).reshape(shape).astype(host.dtype)


def _postprocess_args(postprocess):
    """``postprocess=`` of the validation loops -> keyword arguments of ``keep_components``, or None.  ``"largest"``: the largest
    component of each class under connectivity 1; a dict: any of ``connectivity``, ``keep_largest``, ``min_size``."""
    if postprocess is None:
        return None
    if isinstance(postprocess, str):
        if postprocess != "largest":
            raise ValueError(f"postprocess must be None, 'largest' or a dict of keep_components' keywords, got {postprocess!r}")
        return {"connectivity": 1, "keep_largest": True, "min_size": 0}
    if not isinstance(postprocess, dict) or set(postprocess) - {"connectivity", "keep_largest", "min_size"}:
        raise ValueError(f"postprocess must be None, 'largest' or a dict of keep_components' keywords, got {postprocess!r}")
    kw = {"connectivity": 1, "keep_largest": True, "min_size": 0}
    kw.update(postprocess)
    _components_args(2, kw["connectivity"], kw["keep_largest"], kw["min_size"])
    return kw


def _upload_label(label, device):
    """A host label map as a device tensor of a dtype the metric kernels read (uint8 / bool or int64), or None: the numpy path.
    Floating label maps (MONAI's ``LoadImaged`` yields float32 labels to the AMOS loop) are taken when every value is an integer, for
    which ``label == c`` on the floats and on the integers agree; a map holding any other value (a fraction, NaN, beyond +-2^62) is
    None."""
    label = np.asarray(label.cpu() if torch.is_tensor(label) else label)
    if label.dtype.kind == "f":
        if label.size == 0 or not np.array_equal(label, np.rint(label)):
            return None
        lo, hi = float(label.min()), float(label.max())
        if lo < -2.0 ** 62 or hi > 2.0 ** 62:
            return None
        label = label.astype(np.uint8 if lo >= 0 and hi <= 255 else np.int64)
    elif label.dtype.kind not in "biu":
        return None
    if label.dtype not in (np.bool_, np.uint8, np.int64):
        label = label.astype(np.int64)
    return torch.as_tensor(np.ascontiguousarray(label), device=device)


def _score_prediction(prediction, label, num_classes, dev, voxelspacing=None, post=None, also=None):
    """The per-class list ``[cal_metric(label == c, prediction == c, voxelspacing) for c in 1..num_classes-1]`` of one case, behind the
    optional ``keep_components(prediction, num_classes, **post)`` — the scoring step of the three validation loops (``test_all_case_base``,
    ``test_all_case_amos``, ``val_2D``).  ``prediction``: a tensor on ``dev``, the net's device, or a numpy array; ``label``: a host array or
    tensor.  With ``dev`` a HIP device, ``ICL_VAL_METRICS=device``, 2 <= num_classes <= 256, a label map that ``_upload_label`` takes and
    ``also(gt, prediction, num_classes)`` (the caller's extra condition, if any; asked before a host prediction goes up) both maps are filtered and scored on the
    device (``cal_metric_multiclass``); otherwise on the host, by numpy.  The filter runs once, where the scores are taken."""
    if dev.type == "cuda" and val_metrics_mode() == "device" and 2 <= num_classes <= 256:
        gt = _upload_label(label, dev)      # the ground truth goes up once per case
        if gt is not None and (also is None or also(gt, prediction, num_classes)):
            pred = prediction if torch.is_tensor(prediction) else torch.from_numpy(prediction).to(dev)
            if post is not None:
                pred = keep_components(pred, num_classes, **post)
            return cal_metric_multiclass(gt, pred, num_classes, voxelspacing)
    if torch.is_tensor(prediction):
        prediction = prediction.cpu().numpy()
    if post is not None:
        prediction = keep_components(prediction, num_classes, **post)
    label = np.asarray(label.cpu() if torch.is_tensor(label) else label)
    return [cal_metric(label == c, prediction == c, voxelspacing) for c in range(1, num_classes)]


def test_all_case_base(net, net_type, base_dir, test_list="full_test.list", num_classes=4, patch_size=(48, 160, 160),
                       stride_xy=32, stride_z=24, cases=None, voxelspacing=None, postprocess=None, mirror_axes=None):
    """val_3D.py:100-118.  ``cases`` (iterable of (image, label) numpy pairs, the image [W,H,D] or channel-first [C,W,H,D] beside a
    label [W,H,D]) replaces the h5 files when given; otherwise
    the reference's ``{base_dir}/data/{id}.h5`` layout is read with h5py (not installed in the build image).  ``voxelspacing`` (a number
    or three, the voxel size along the label map's axes) gives HD95 in its units (``cal_metric_multiclass``); None: voxels, as the reference.
    ``postprocess``: None (the reference), ``"largest"`` or a dict of ``keep_components``' keywords — the predicted label map goes through
    ``keep_components`` before it is scored (on the device when it is there).  ``mirror_axes``: None (the reference) or the axes out of
    0, 1, 2 of mirror test-time augmentation — every window is predicted once per subset of them, at one forward per pass
    (``test_single_case_base``)."""
    if voxelspacing is not None:
        voxelspacing = _normalize_spacing(voxelspacing)
    post = _postprocess_args(postprocess)
    _mirror_masks(mirror_axes)
    if cases is None:
        import h5py  # noqa: F401 — same dependency as the reference
        with open(base_dir + "/{}".format(test_list), "r") as f:
            ids = [ln.strip().split(",")[0] for ln in f if ln.strip()]

        def _gen():
            for i in ids:
                with h5py.File(base_dir + "/data/{}.h5".format(i), "r") as h5f:
                    yield h5f["image"][:], h5f["label"][:]
        cases = _gen()
    metric_cal = [[] for _ in range(num_classes - 1)]
    dev = next(net.parameters()).device
    for image, label in cases:      # the label map stays on the net's device up to its scores
        prediction, _ = _single_case_on_device(net, net_type, image, stride_xy, stride_z, patch_size, num_classes, want_score=False,
                                               mirror_axes=mirror_axes)
        for i, m in enumerate(_score_prediction(prediction, label, num_classes, dev, voxelspacing, post)):
            metric_cal[i].append(m)
    return metric_cal


# --------------------------------------------------------------------------------------------------------------------
# AMOS validation: MONAI-style sliding window (val_3D.py:120-137)
# --------------------------------------------------------------------------------------------------------------------

def _scan_starts(size: int, roi: int, overlap: float):
    """Window origins along one axis as MONAI 1.0.1 ``sliding_window_inference`` places them (``_get_scan_interval`` +
    ``dense_patch_slices``): stride ``int(roi * (1 - overlap))`` (the whole axis when it equals the window), ``ceil((size - roi) /
    stride) + 1`` windows, the last ones shifted back inside the volume."""
    if size == roi:
        return [0]
    interval = int(roi * (1 - overlap))
    interval = interval if interval > 0 else 1
    num = int(math.ceil(float(size - roi) / interval)) + 1
    return [i * interval - max(i * interval + roi - size, 0) for i in range(num)]


@torch.no_grad()
def sliding_window_inference(inputs, roi_size, sw_batch_size, predictor, overlap: float = 0.25, mode="constant", sigma_scale=0.125,
                             mirror_axes=None, **kwargs):
    """Restatement of ``monai.inferers.sliding_window_inference(inputs, roi_size, sw_batch_size, predictor, overlap=0.25,
    mode="constant", sigma_scale=0.125)`` as the reference calls it (val_3D.py:130-132): symmetric zero padding of volumes smaller than the
    window, the window grid of ``_scan_starts``, ``sw_batch_size`` windows per forward, predictor OUTPUTS (logits) averaged over
    overlapping windows, padding cropped off again.  ``mode="constant"`` weights every window voxel alike; ``mode="gaussian"`` weights it
    with ``gaussian_importance_map(roi_size, sigma_scale)``, which follows MONAI's Gaussian mode (MONAI filters a delta with an
    erf-integrated kernel; see there) — any other mode is a ValueError.  Everything stays on the device of ``inputs``; an fp32 tensor on a
    HIP device goes through the window kernels (``ICL_VAL_WINDOWS``), anything else, and a predictor whose output extent differs from the
    window's, through the ATen loop below.  ``mirror_axes`` (not MONAI's): None, or the axes out of 0, 1, 2 (the three spatial axes of a
    3-D input) of mirror test-time augmentation — ``sw_batch_size`` then counts passes (``_run_windows``); it is not handed to the
    predictor.  MONAI is not installed in the build image: parity unpinned."""
    masks = _mirror_masks(mirror_axes)
    b = inputs.shape[0]
    size = list(inputs.shape[2:])
    if masks is not None and len(size) != 3:
        raise ValueError(f"mirror_axes needs a 3-D input [B, C, D, H, W], got shape {tuple(inputs.shape)}")
    roi = [int(r) for r in roi_size]
    imp = _importance_map(mode, roi, sigma_scale, inputs.device)
    pads = []
    for s, r in zip(size, roi):
        diff = max(r - s, 0)
        pads.append((diff // 2, diff - diff // 2))
    psize = [s + a + c for s, (a, c) in zip(size, pads)]
    grids = [_scan_starts(s, r, overlap) for s, r in zip(psize, roi)]
    starts = [(bi, z, y, x) for bi in range(b) for z in grids[0] for y in grids[1] for x in grids[2]]
    (_, out), _ = _run_windows(
        inputs, roi, pads, psize, starts, sw_batch_size, lambda win: predictor(win, **kwargs), imp, False, "quotients",
        _window_kernels_apply(inputs) and len(size) == 3, _fits_amos(roi, inputs.device), masks=masks)
    return out


def test_all_case_amos(net, net_type, val_loader, num_classes=4, voxelspacing=None, postprocess=None, mirror_axes=None):
    """val_3D.py:120-137: every validation volume through ``sliding_window_inference(image, (96, 96, 96), 4, net[, inference=True])``,
    argmax over the averaged logits, ``cal_metric`` per foreground class.  The reference wraps the inference in fp16 autocast; the
    HIP kernels compute in fp32 (a strictly more accurate evaluation of the same network).  ``voxelspacing`` (a number or three: the voxel
    size along D, H, W) gives HD95 in its units; the loop scores [1, D, H, W] maps, on which every voxel of a class is a border voxel,
    and those take the numpy path when a spacing is given (the surface kernels take 3-D maps).  ``postprocess``: as in
    ``test_all_case_base``; the [1, D, H, W] prediction is filtered as the 3-D map behind its leading axis.  ``mirror_axes``: None, or the
    axes out of 0, 1, 2 (D, H, W) of mirror test-time augmentation (``sliding_window_inference``)."""
    if voxelspacing is not None:
        voxelspacing = _normalize_spacing(voxelspacing)
    post = _postprocess_args(postprocess)
    _mirror_masks(mirror_axes)
    metric_cal = [[] for _ in range(num_classes - 1)]
    net.eval()
    dev = next(net.parameters()).device
    for batch in val_loader:
        image, label = batch["image"].to(dev), batch["label"].squeeze(0)
        kw = {"inference": True} if net_type in ("unet_3D_icl", "swinunetr_icl") else {}
        logits = sliding_window_inference(image, (96, 96, 96), 4, net, mirror_axes=mirror_axes, **kw)
        prediction = torch.argmax(logits, dim=1)
        for i, m in enumerate(_score_prediction(prediction, label, num_classes, dev, voxelspacing, post, also=_device_metrics_apply)):
            metric_cal[i].append(m)
    return metric_cal
