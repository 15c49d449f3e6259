"""numpy restatement of the multi-modal feed (DESIGN.md §2 "Multi-modal feed"), shared by tests/test_multimodal_feed_emu.py (the kernel
sources on the CPU emulation), tests/test_multimodal_host.py and tests/test_gpu_multimodal.py (the library on the GPU):

* the forward chain of the gather, per channel:  flip(rot90(x, k), axis) -> zero padding -> crop  (icl_crop_rotflip_channels);
* the channel-wise normalisation (icl_channel_norm_stats / icl_channel_norm_apply);
* the window loop of the BraTS validation on a channel-first case.

Nothing here reads the kernels' code or the reference tree.  Parity with MONAI's own NormalizeIntensityd is unpinned (MONAI is not installed)."""
import ctypes

import numpy as np
import torch

SOURCES = [(7, 9, 5), (9, 7, 8), (5, 6, 8)]      # the last: every axis <= the patch, so the padding rule fires for both patches
PATCH_SCALAR = (6, 6, 5)                         # o2 % 4 != 0: one voxel per thread
PATCH_QUAD = (6, 6, 8)                           # o2 % 4 == 0: one quad per thread
ROTFLIPS = [(k, axis) for k in range(4) for axis in (-1, 0, 1)]

# The step test's band for the gradient of conv1.conv1.0.weight at in_channels = 4 (tests/test_gpu_multimodal.py): four times the error
# of the oracle's own fp32 evaluation against its fp64 evaluation, max |difference| / max |value|, on the test's inputs (small
# unet_3D_icl, n_classes 2, in_channels 4, resolutions (2, 4, 8), volume seed 1337, label seed 4242, hash-filled parameters).  Obtained
# on the CPU with oracle_grad_error() below (torch CPU, fp32 against fp64); profiles/multimodal.md records the run.  It is a margin
# over the reference's own rounding error, never over the code under test.
ORACLE_FP32_GRAD_ERROR = 5.14e-6      # oracle_grad_error() returned 5.144961e-06
GRAD_BAND_FACTOR = 4.0


def source_volume(shape, channels, tag=0):
    """image fp32 [channels, *shape] (or [*shape] with channels None): channel c holds 1000 c + voxel index + 1 (never 0, so a zero
    is a padded voxel), so a channel taken from the wrong plane or a stride off by one cannot go unnoticed.  label uint8 [*shape]."""
    n = int(np.prod(shape))
    index = np.arange(n, dtype=np.float32).reshape(shape)
    if channels is None:
        image = index + 1.0 + 100000.0 * tag
    else:
        image = np.stack([1000.0 * c + index + 1.0 + 100000.0 * tag for c in range(channels)]).astype(np.float32)
    label = ((np.arange(n) * 7 + 3 * tag) % 5 + 1).astype(np.uint8).reshape(shape)
    return np.ascontiguousarray(image, dtype=np.float32), label


def pads_for(shape, k, patch):
    """RandomCrop's padding rule on the extents after rot90."""
    dims = [shape[1], shape[0], shape[2]] if k & 1 else list(shape)
    pads = [0, 0, 0]
    if any(dims[a] <= patch[a] for a in range(3)):
        pads = [max((patch[a] - dims[a]) // 2 + 3, 0) for a in range(3)]
    return dims, pads


def chain(vol, row, patch):
    """One 3-D array through the forward chain of a parameter row (n0, n1, n2, k, axis, p0, p1, p2, c0, c1, c2)."""
    k, axis = row[3], row[4]
    x = np.rot90(vol, k)
    if axis >= 0:
        x = np.flip(x, axis=axis)
    x = np.pad(x, [(p, p) for p in row[5:8]], mode="constant", constant_values=0)
    c = row[8:11]
    out = x[c[0]:c[0] + patch[0], c[1]:c[1] + patch[1], c[2]:c[2] + patch[2]]
    assert out.shape == tuple(patch), (out.shape, row)
    return out


def sweep_rows(patch, seed=5):
    """(source index, row) for every source, k and flip axis, and for up to six origins of the depth axis each — consecutive ones, so
    that the last coordinate minus the padding is a multiple of 4 in some samples and not in others; the other two origins vary with a
    fixed generator.  Ordered so that neighbouring samples come from different sources (mixed launches)."""
    rng = np.random.RandomState(seed)
    per_source = []
    for si, shape in enumerate(SOURCES):
        rows = []
        for k, axis in ROTFLIPS:
            dims, pads = pads_for(shape, k, patch)
            span = [dims[a] + 2 * pads[a] - patch[a] for a in range(3)]      # randint(0, span): origins 0 .. span - 1
            assert min(span) >= 1
            for c2 in range(min(span[2], 6)):
                rows.append((si, (*shape, k, axis, *pads, int(rng.randint(0, span[0])), int(rng.randint(0, span[1])), c2)))
        per_source.append(rows)
    out = []
    for j in range(max(len(r) for r in per_source)):
        out += [r[j] for r in per_source if j < len(r)]
    aligned = [(row[10] - row[7]) % 4 == 0 for _, row in out]
    assert any(aligned) and not all(aligned)
    return out


def make_store_arrays(channels):
    """[(image [channels, *shape] or [*shape], label)] of the three sources."""
    return [source_volume(shape, channels, tag) for tag, shape in enumerate(SOURCES)]


def expected(volumes, items, patch):
    """(image [n, C, *patch] fp32, label [n, *patch] int64) of the chain over `items` = [(source index, row)]."""
    images, labels = [], []
    for si, row in items:
        image, label = volumes[si]
        planes = image if image.ndim == 4 else image[None]
        images.append(np.stack([chain(p, row, patch) for p in planes]))
        labels.append(chain(label, row, patch).astype(np.int64))
    return np.stack(images).astype(np.float32), np.stack(labels)


_KEEP = []


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream) if dev.type == "cuda" else None


def raw_channels(lib, tensors, items, channels, patch, misaligned=False, batch=None, null=None, entry="icl_crop_rotflip_channels"):
    """One launch of the entry through ctypes on sentinel-filled outputs.  tensors: [(image tensor, label tensor)] on the device;
    misaligned: the image output starts 4 bytes past a 16-byte boundary.  Returns (rc, image [m, C, *patch], label [m, *patch])."""
    m = len(items)
    dev = tensors[0][0].device
    ptrs = ctypes.c_void_p * m
    held = max(channels, 1)                         # a refused channel count still gets a real output pointer
    numel = m * held * max(int(np.prod(patch)), 1)
    buf = torch.full((numel + 4,), -7.0, dtype=torch.float32, device=dev)
    image = buf[1:1 + numel] if misaligned else buf[:numel]
    assert image.data_ptr() % 16 == (4 if misaligned else 0)
    label = torch.full((m * max(int(np.prod(patch)), 1),), -7, dtype=torch.int64, device=dev)
    if int(np.prod(patch)) > 0:
        image, label = image.view(m, held, *patch), label.view(m, *patch)
    args = [ptrs(*[tensors[si][0].data_ptr() for si, _ in items]), ptrs(*[tensors[si][1].data_ptr() for si, _ in items]),
            (ctypes.c_int32 * (11 * m))(*[int(v) for _, row in items for v in row])]
    outs = [image.data_ptr(), label.data_ptr()]
    if null is not None:
        if null < 3:
            args[null] = None
        else:
            outs[null - 3] = None
    _KEEP.append((args, buf, label))
    count = m if batch is None else batch
    if entry == "icl_crop_rotflip":
        rc = lib.icl_crop_rotflip(*args, count, *outs, *patch, _stream(dev))
    else:
        rc = lib.icl_crop_rotflip_channels(*args, count, channels, *outs, *patch, _stream(dev))
    return rc, image, label


def check_sweep(lib, device, channels, patch, per_launch=16, misaligned=False):
    """The sweep through the raw entry in launches of `per_launch` mixed samples; every output channel and the label against the
    chain, exactly; with one channel also against icl_crop_rotflip on the same memory, bit for bit.  Returns the number of samples."""
    volumes = make_store_arrays(channels)
    tensors = [(torch.as_tensor(i).to(device), torch.as_tensor(l).to(device)) for i, l in volumes]
    items = sweep_rows(patch)
    want_image, want_label = expected(volumes, items, patch)
    for lo in range(0, len(items), per_launch):
        part = items[lo:lo + per_launch]
        rc, image, label = raw_channels(lib, tensors, part, channels, patch, misaligned)
        assert rc == 0, lib.icl_last_error()
        got_image, got_label = image.cpu().numpy(), label.cpu().numpy()
        for j in range(len(part)):
            for c in range(channels):
                assert np.array_equal(got_image[j, c], want_image[lo + j, c]), (part[j], c, channels, patch)
            assert np.array_equal(got_label[j], want_label[lo + j]), (part[j], channels, patch)
        if channels == 1:
            rc, one_image, one_label = raw_channels(lib, tensors, part, 1, patch, misaligned, entry="icl_crop_rotflip")
            assert rc == 0
            assert torch.equal(one_image.view(torch.int32), image.view(torch.int32)) and torch.equal(one_label, label)
    _KEEP.clear()
    return len(items)


# ---- channel-wise normalisation --------------------------------------------------------------------------------------------------

NORM_MASKS = ("nonzero", "positive", "all")
NORM_APPLY = ("mask", "all")


def norm_fixture(shape=(3, 5, 6, 8), seed=11):
    """Integer-valued intensities (MR data is integer: every sum is exact in double) with a zero background and some negative voxels.
    Channel 0: mixed; channel 1: entirely zero; channel 2: constant 7 on the foreground.  More channels repeat channel 0's recipe."""
    rng = np.random.RandomState(seed)
    x = np.zeros(shape, dtype=np.float32)
    for c in range(shape[0]):
        v = rng.randint(-40, 900, size=shape[1:]).astype(np.float32)
        v[rng.rand(*shape[1:]) < 0.35] = 0.0
        x[c] = v
    x[1] = 0.0
    x[2] = np.where(x[0] != 0, 7.0, 0.0)
    return x


def norm_mask(x, mask):
    return {"nonzero": x != 0, "positive": x > 0, "all": np.ones(x.shape, dtype=bool)}[mask]


def norm_reference(x, mask, apply_to):
    """(normalised volume fp32, stats float64 [C, 3] = count, mean, std) by numpy: float64 statistics of the masked voxels, rounded to
    fp32, std 0 -> 1, then (x - m) / s in fp32 on the mask or everywhere; an empty mask leaves the channel untouched."""
    out = x.copy()
    stats = np.zeros((x.shape[0], 3))
    for c in range(x.shape[0]):
        sel = norm_mask(x[c], mask)
        if not sel.any():
            continue
        vals = x[c][sel].astype(np.float64)
        m, s = vals.mean(), vals.std()
        stats[c] = (vals.size, m, s)
        m32, s32 = np.float32(m), np.float32(s)
        if s32 == 0:
            s32 = np.float32(1.0)
        where = sel if apply_to == "mask" else np.ones(sel.shape, dtype=bool)
        z = (x[c] - m32) / s32
        assert z.dtype == np.float32
        out[c][where] = z[where]
    return out, stats


def no_fp32_tie(value, rel):
    """True when every double within `rel` (relative) of `value` rounds to the same fp32: no rounding tie can make two evaluations
    that agree to `rel` differ after the rounding to fp32."""
    return np.float32(value * (1.0 - rel)) == np.float32(value * (1.0 + rel))


# ---- validation: the window loop of test_single_case_base on a channel-first case ---------------------------------------------------

class PerVoxelNet(torch.nn.Module):
    """Stand-in net: three logits that are a fixed per-voxel function of the input channels (the first and the last: both channels of
    a two-channel case, the one channel of a [W,H,D] case twice).  With integer inputs the logits are an integer, a half-integer and
    a quarter-integer, so no two are ever closer than 0.25: the arg-max does not hang on the last bit of a soft-max."""

    def __init__(self):
        super().__init__()
        self.anchor = torch.nn.Parameter(torch.zeros(1))
        self.seen = []

    def forward(self, win):
        self.seen.append(tuple(win.shape))
        a, b = win[:, 0], win[:, -1]
        return torch.stack([a - b, b - 0.5, 0.25 - a], dim=1)


def per_voxel_logits(win):
    a, b = win[0], win[-1]
    return np.stack([a - b, b - 0.5, 0.25 - a])


def window_loop_reference(image, patch, stride_xy, stride_z):
    """The BraTS validation loop restated: symmetric zero padding to the patch, windows on the strided grid with the last one clamped,
    mean of the soft-max over the windows covering a voxel, arg-max, crop.  image [C, W, H, D] (or [W, H, D])."""
    vol = image if image.ndim == 4 else image[None]
    pads = []
    for dim, p in zip(vol.shape[1:], patch):
        tot = max(p - dim, 0)
        pads.append((tot // 2, tot - tot // 2))
    x = np.pad(vol, [(0, 0)] + pads, mode="constant").astype(np.float32)
    ww, hh, dd = x.shape[1:]
    score = np.zeros((3, ww, hh, dd), dtype=np.float64)
    count = np.zeros((ww, hh, dd), dtype=np.float64)
    windows = 0
    for ix in range(int(np.ceil((ww - patch[0]) / stride_xy)) + 1):
        xs = min(stride_xy * ix, ww - patch[0])
        for iy in range(int(np.ceil((hh - patch[1]) / stride_xy)) + 1):
            ys = min(stride_xy * iy, hh - patch[1])
            for iz in range(int(np.ceil((dd - patch[2]) / stride_z)) + 1):
                zs = min(stride_z * iz, dd - patch[2])
                sl = (slice(xs, xs + patch[0]), slice(ys, ys + patch[1]), slice(zs, zs + patch[2]))
                logits = per_voxel_logits(x[(slice(None),) + sl]).astype(np.float64)
                e = np.exp(logits - logits.max(axis=0, keepdims=True))
                score[(slice(None),) + sl] += e / e.sum(axis=0, keepdims=True)
                count[sl] += 1
                windows += 1
    label = np.argmax(score / count, axis=0)
    crop = tuple(slice(p[0], p[0] + n) for p, n in zip(pads, vol.shape[1:]))
    return label[crop].astype(np.int64), windows


def validation_case(shape, seed=3):
    """Small integers, channel-first."""
    return np.random.RandomState(seed).randint(-3, 4, size=shape).astype(np.float32)


# ---- the step at in_channels = 4 ---------------------------------------------------------------------------------------------------

STEP_CLASSES, STEP_CHANNELS, STEP_RES, STEP_SIZE = 2, 4, (2, 4, 8), (32, 32, 32)


def step_inputs():
    from icl_amd.utils.hashfill import synthetic_labels, synthetic_volume
    return synthetic_volume((2, STEP_CHANNELS, *STEP_SIZE), 1337), synthetic_labels((1, *STEP_SIZE), 4242, STEP_CLASSES)


def oracle_step(dtype=torch.float32):
    """The oracle's forward, losses and the gradient of conv1.conv1.0.weight for the step test's model and batch, on the CPU in `dtype`.
    Returns (outputs, total loss, loss parts, gradient)."""
    from oracle import icl_oracle as O
    f = (256, 128, 64)
    shapes = (O.backbone_shapes(STEP_CLASSES, STEP_CHANNELS)
              + O.aligner_shapes("sspa.", f, STEP_RES, STEP_CLASSES, O.UNET3D_HEADS)
              + O.aligner_shapes("uscl.", f, STEP_RES, STEP_CLASSES, O.UNET3D_HEADS))
    p = {k: v.to(dtype) for k, v in O.make_params(shapes).items()}
    p.update({k: v.to(dtype) for k, v in O.aligner_buffers("sspa.", O.UNET3D_HEADS).items()})
    p.update({k: v.to(dtype) for k, v in O.aligner_buffers("uscl.", O.UNET3D_HEADS).items()})
    w = p["conv1.conv1.0.weight"].requires_grad_()
    vol, lab = step_inputs()
    vol = vol.to(dtype)
    outs = O.unet_3d_icl_forward(p, vol[:1], vol[1:])
    total, parts = O.icl_losses(outs, lab, STEP_CLASSES, size=STEP_SIZE)
    total.backward()
    return outs, total.detach(), {k: v.detach() for k, v in parts.items()}, w.grad.detach()


def oracle_grad_error():
    """max |fp32 - fp64| / max |fp64| of the oracle's gradient of conv1.conv1.0.weight: the figure ORACLE_FP32_GRAD_ERROR records."""
    g32, g64 = oracle_step(torch.float32)[3], oracle_step(torch.float64)[3]
    return float((g32.double() - g64).abs().max() / g64.abs().max())
