"""Shared inputs, yardstick and checks of the AMOS cached-prefix tests (tests/test_amos_prefix_host.py, tests/test_amos_prefix_emu.py on the
CPU emulator, tests/test_gpu_amos_prefix.py on the GPU; icl_amd/csrc/kernels/prefix.h, icl_amd/dataloaders/amos.py).  Not a test module.

``forward_chain`` is the yardstick: a numpy restatement of ScaleIntensityRanged -> CropForegroundd -> Orientationd("RAS") -> [SpatialPadd]
-> Spacingd as the LITERAL chain — window the whole volume, ``np.argwhere`` box, ``np.transpose`` / ``np.flip``, ``np.pad``, per-axis tap
tables and the eight-term sum in the documented order — deliberately the opposite formulation from the kernel, which composes all of it
into one gather from the raw arrays.  ``inverse_chain`` is the inverse for label maps, again literal: resample onto the padded oriented
grid, cut the pad off, flip back, transpose back, paste into a zero volume.  Every comparison against them is exact (``np.array_equal``):
both sides perform the same IEEE operations in the same order.  MONAI and nibabel are not installed, so this restates the published
definitions of MONAI 1.0.1 and of nibabel's ``io_orientation``; parity with MONAI's own code is unpinned (DESIGN.md "AMOS cached prefix").

The orientation enters the yardstick as a (perm, sign) table that the case list states outright; ``orientation_from_affine`` is held to
those tables in test_amos_prefix_host.py.  References are computed once per case and shared.
"""
import functools
import itertools

import numpy as np
import torch

from icl_amd.dataloaders.amos import amos_prefix, restore_label

WINDOW = (-175.0, 250.0, 0.0, 1.0, True)
PIXDIM = (1.5, 1.5, 2.0)
RAWS = [(7, 5, 9), (12, 11, 4), (9, 9, 8)]
# per ORIENTED axis: downsample on axes 0, 1 and upsample on axis 2 | coordinates on half-integers on axis 0 (label ties), upsample on
# axes 1, 2 | leave alone
SPACINGS = [(0.8, 0.8, 5.0), (3.0, 0.75, 1.0), (1.5, 1.5, 2.0)]
ORIENTATIONS = [(perm, sign) for perm in itertools.permutations(range(3)) for sign in itertools.product((1, -1), repeat=3)]      # all 48
assert len(ORIENTATIONS) == 48 and ORIENTATIONS[0] == ((0, 1, 2), (1, 1, 1))
BOX_KINDS = ("inside", "faces", "voxel", "flat")
MID_RAW = (96, 80, 40)


def box_of(shape, kind):
    """(lo, hi) of the foreground the raw volume is given, hi exclusive: strictly inside | touching every face | a single voxel | extent 1
    on one axis only."""
    n = shape
    if kind == "inside":
        return tuple(1 for _ in n), tuple(v - 1 for v in n)
    if kind == "faces":
        return (0, 0, 0), tuple(n)
    if kind == "voxel":
        lo = tuple(v // 2 for v in n)
        return lo, tuple(v + 1 for v in lo)
    if kind == "flat":
        return (1, n[1] // 2, 0), (n[0], n[1] // 2 + 1, n[2] - 1)
    if kind == "small":                                  # for pad_to: at most 5 voxels an axis
        lo = tuple(min(1, v - 1) for v in n)
        return lo, tuple(min(l + 5, v) for l, v in zip(lo, n))
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def raw_volume(shape, kind, seed=0):
    """(image fp32 in Hounsfield-like units, label uint8) whose foreground box (windowed value > 0) is exactly ``box_of(shape, kind)``:
    -500 outside; inside, values in (-175, 400) — some above the window, which clip to 1 — with a fifth of the voxels knocked back to
    -300, the box's two extreme corners excepted.  The label is random 0..15 everywhere, outside the box too."""
    rng = np.random.RandomState(1000 + seed + 7 * ("inside", "faces", "voxel", "flat", "small").index(kind))
    lo, hi = box_of(shape, kind)
    image = np.full(shape, -500.0, dtype=np.float32)
    region = tuple(slice(a, b) for a, b in zip(lo, hi))
    inner = rng.uniform(-174.0, 400.0, size=tuple(b - a for a, b in zip(lo, hi))).astype(np.float32)
    holes = rng.rand(*inner.shape) < 0.2
    holes[0, 0, 0] = holes[-1, -1, -1] = False
    inner[holes] = -300.0
    image[region] = inner
    label = rng.randint(0, 16, size=shape).astype(np.uint8)
    return image, label


def source_spacing(perm, oriented_spacing):
    """Voxel sizes per SOURCE axis such that oriented axis a (source axis perm[a]) has oriented_spacing[a]."""
    z = [0.0, 0.0, 0.0]
    for a in range(3):
        z[perm[a]] = oriented_spacing[a]
    return tuple(z)


def affine_of(perm, sign, oriented_spacing, tilt_degrees=0.0, origin=(-12.5, 30.0, 7.25)):
    """A 4x4 affine whose source axis perm[a] runs along RAS axis a (backwards for sign[a] == -1) with the given voxel size, optionally
    tilted by a rotation about the (1, 1, 1) direction."""
    A = np.zeros((4, 4))
    for a in range(3):
        A[a, perm[a]] = sign[a] * oriented_spacing[a]
    if tilt_degrees:
        t = np.deg2rad(tilt_degrees)
        k = np.ones(3) / np.sqrt(3.0)
        K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        A[:3, :3] = (np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)) @ A[:3, :3]
    A[:3, 3] = origin
    A[3, 3] = 1.0
    return A


def axcodes_of(perm, sign):
    letters = (("L", "R"), ("P", "A"), ("I", "S"))
    codes = [None] * 3
    for a in range(3):
        codes[perm[a]] = letters[a][sign[a] > 0]
    return "".join(codes)


# ---- the yardstick ----------------------------------------------------------------------------------------------------------------------

def window_volume(image, window=WINDOW):
    a_min, a_max, b_min, b_max, clip = window
    v = np.asarray(image, dtype=np.float32)
    t = (v - np.float32(a_min)) / np.float32(float(a_max) - float(a_min))
    t = t * np.float32(float(b_max) - float(b_min))
    t = t + np.float32(b_min)
    if clip:
        t = np.minimum(np.maximum(t, np.float32(b_min)), np.float32(b_max))
    assert t.dtype == np.float32
    return t


def foreground_box(windowed):
    where = np.argwhere(windowed > 0)
    if where.shape[0] == 0:
        raise ValueError("no foreground")
    return tuple(int(v) for v in where.min(0)), tuple(int(v) + 1 for v in where.max(0))


def orient(x, perm, sign):
    x = np.transpose(x, perm)
    for a in range(3):
        if sign[a] < 0:
            x = np.flip(x, a)
    return x


def pad_widths(extents, pad_to):
    if pad_to is None:
        return [(0, 0)] * 3
    w = [max(int(t) - e, 0) for t, e in zip(pad_to, extents)]
    return [(v // 2, v - v // 2) for v in w]


def out_extent(m, s, p):
    return int(np.rint(np.float64(m - 1) * (np.float64(s) / np.float64(p)) + 1.0))


def tap_table(o, m, s, p):
    """Per output index of one axis: (x fp64, i0, i1, w0, w1, nearest)."""
    x = np.arange(o, dtype=np.float64) * (np.float64(p) / np.float64(s))
    x = np.minimum(np.maximum(x, 0.0), np.float64(m - 1))
    fl = np.floor(x)
    f = x - fl
    i0 = fl.astype(np.int64)
    i1 = np.minimum(i0 + 1, m - 1)
    return x, i0, i1, 1.0 - f, f, np.rint(x).astype(np.int64)


def respace(image, label, spacing, pixdim):
    """Spacing(diagonal=False, padding_mode="border") of the oriented (padded) pair: bilinear image fp32, nearest label."""
    m = image.shape
    o = tuple(out_extent(m[a], spacing[a], pixdim[a]) for a in range(3))
    taps = [tap_table(o[a], m[a], spacing[a], pixdim[a]) for a in range(3)]
    xd = image.astype(np.float64)
    acc = None
    for b0, b1, b2 in itertools.product((0, 1), repeat=3):          # (0,0,0), (0,0,1), (0,1,0), ..., (1,1,1)
        tap = xd[np.ix_(taps[0][1 + b0], taps[1][1 + b1], taps[2][1 + b2])]
        w = (taps[0][3 + b0][:, None, None] * taps[1][3 + b1][None, :, None]) * taps[2][3 + b2][None, None, :]
        term = tap * w
        acc = term if acc is None else acc + term
    near = label[np.ix_(taps[0][5], taps[1][5], taps[2][5])]
    return acc.astype(np.float32), np.ascontiguousarray(near), taps


def forward_chain(image, label, perm, sign, spacing, pixdim=PIXDIM, pad_to=None, window=WINDOW):
    """(image_t fp32 [o], label_t uint8 [o], stages): ``spacing`` per ORIENTED axis.  ``stages``: the box, the windowed oriented padded
    crop (image, label) and the tap tables, for the checks that look inside."""
    w = window_volume(image, window)
    lo, hi = foreground_box(w)
    region = tuple(slice(a, b) for a, b in zip(lo, hi))
    xi, xl = orient(w[region], perm, sign), orient(np.asarray(label)[region], perm, sign)
    widths = pad_widths(xi.shape, pad_to)
    xi = np.pad(xi, widths, mode="constant", constant_values=0.0)
    xl = np.pad(xl, widths, mode="constant", constant_values=0)
    out_i, out_l, taps = respace(xi, xl, spacing, pixdim)
    return out_i, out_l.astype(np.uint8), {"box": (lo, hi), "oriented": (np.ascontiguousarray(xi), np.ascontiguousarray(xl)),
                                           "widths": widths, "taps": taps}


def inverse_chain(prediction, shape, box, perm, sign, spacing, pixdim, widths):
    """The inverse for a label map on the respaced grid -> uint8 on the raw grid, as its own literal chain."""
    lo, hi = box
    e = [hi[perm[a]] - lo[perm[a]] for a in range(3)]
    m = [widths[a][0] + e[a] + widths[a][1] for a in range(3)]
    o = prediction.shape
    index = []
    for a in range(3):
        y = np.arange(m[a], dtype=np.float64) * (np.float64(spacing[a]) / np.float64(pixdim[a]))
        y = np.minimum(np.maximum(y, 0.0), np.float64(o[a] - 1))
        index.append(np.rint(y).astype(np.int64))
    z = np.asarray(prediction)[np.ix_(*index)]                                           # back on the padded oriented grid
    z = z[tuple(slice(widths[a][0], widths[a][0] + e[a]) for a in range(3))]             # the pad comes off
    for a in range(3):
        if sign[a] < 0:
            z = np.flip(z, a)
    z = np.transpose(z, np.argsort(perm))                                                # raw axes again
    out = np.zeros(shape, dtype=np.uint8)
    out[tuple(slice(a, b) for a, b in zip(lo, hi))] = z.astype(np.uint8)
    return out


# ---- the shared case list -------------------------------------------------------------------------------------------------------------

def make_case(raw, kind, orientation, spacing, pad_to=None, pixdim=PIXDIM, route="affine", seed=0):
    return {"raw": raw, "kind": kind, "perm": orientation[0], "sign": orientation[1], "spacing": spacing, "pixdim": pixdim, "pad_to": pad_to,
            "route": route, "seed": seed}


def _cases():
    cases = []
    # all 48 orientations on the first raw volume; the box kind and the spacing walk through their values, the route alternates
    for i, ori in enumerate(ORIENTATIONS):
        cases.append(make_case(RAWS[0], BOX_KINDS[i % 3], ori, SPACINGS[(i // 3) % 3], route=("affine", "axcodes")[i % 2]))
    # a handful on the others: every box kind x every spacing
    picks = [ORIENTATIONS[0], ORIENTATIONS[7], ORIENTATIONS[13], ORIENTATIONS[22], ORIENTATIONS[35], ORIENTATIONS[41], ORIENTATIONS[47]]
    for r, raw in enumerate(RAWS[1:]):
        for i, (kind, spacing) in enumerate(itertools.product(BOX_KINDS[:3], SPACINGS)):
            cases.append(make_case(raw, kind, picks[(i + 3 * r) % len(picks)], spacing, route=("axcodes", "affine")[i % 2]))
    # a box of extent 1 on one axis, under three orientations and every spacing
    for i, spacing in enumerate(SPACINGS):
        cases.append(make_case(RAWS[i], "flat", ORIENTATIONS[(0, 19, 44)[i]], spacing))
    # SpatialPad before the respacing: a box of at most 5 voxels an axis -> (10, 10, 10), and a pad on some axes only
    for i, spacing in enumerate(SPACINGS):
        cases.append(make_case(RAWS[i], "small", ORIENTATIONS[(0, 29, 10)[i]], spacing, pad_to=(10, 10, 10)))
    cases.append(make_case(RAWS[1], "faces", ORIENTATIONS[0], SPACINGS[2], pad_to=(10, 10, 10)))         # extents 12, 11 stay, 4 -> 10
    cases.append(make_case(RAWS[0], "voxel", ORIENTATIONS[5], SPACINGS[0], pad_to=(10, 10, 10)))
    return cases


CASES = _cases()
QUAD_CASE = make_case(RAWS[2], "faces", ORIENTATIONS[0], SPACINGS[2])                   # o = (9, 9, 8): o2 % 4 == 0, four outputs a thread
QUAD_CASE_RESCALED = make_case(RAWS[0], "faces", ORIENTATIONS[0], (0.8, 0.8, 2.75))     # o2 = rint(8 * 1.375 + 1) = 12, a real rescale
QUAD_CASE_REVERSED = make_case(RAWS[2], "inside", ORIENTATIONS[7], (0.8, 0.8, 3.0))     # axes reversed; o2 = rint(5 * 1.5 + 1) = 8 (half to even)
# The resample kernel cuts oriented axis 2 into tiles of at most 512 outputs whose taps span at most 256 slots (kPrefixTile2,
# kPrefixSlots of prefix.h): more than one tile along that axis, with and without the four-outputs-a-thread path.
TILE_CASES = [
    make_case((3, 3, 600), "faces", ORIENTATIONS[0], PIXDIM),                            # o2 = 600: 253 slots' worth a tile, 252 for quads: 252 + 252 + 96
    make_case((3, 3, 601), "faces", ORIENTATIONS[2], PIXDIM),                            # o2 = 601: one output a thread, axis 1 reversed
    # p / s = 2 on axis 2: 252 / 2 + 1 = 127 outputs a tile, 124 for quads; o2 = rint(702 / 2 + 1) = 352 -> 124 + 124 + 104, all reversed
    make_case((3, 3, 703), "faces", ORIENTATIONS[7], (1.5, 1.5, 1.0)),
    # p / s = 3.3: 77 outputs a tile; oriented axis 2 is raw axis 0, reversed (strided reads); o2 = rint(699 / 3.3 + 1) = 213 -> 77 + 77 + 59
    make_case((700, 3, 3), "faces", ORIENTATIONS[29], (1.5, 1.5, 2.0 / 3.3), route="axcodes"),
    make_case((3, 4, 300), "inside", ORIENTATIONS[5], (1.5, 1.5, 5.0)),                  # 2.5 x up: o2 = rint(297 * 2.5 + 1) = 744: 512 + 232
    make_case((3, 3, 200), "small", ORIENTATIONS[0], (0.8, 0.8, 4.0), pad_to=(5, 5, 900)),   # padded to 900 slots, o2 = rint(899 * 2 + 1) = 1799
]
# 1,100 x 61 x 1 = 67,100 tiles, more than the resample grid's 65,536 workgroups, and 2,116,400 raw voxels, more than the restore grid's
# 8,192 x 256 threads: both kernels' outer loops run a second time
MANY_TILES_CASE = make_case((1100, 481, 4), "faces", ORIENTATIONS[0], PIXDIM, seed=11)
MID_CASE = make_case(MID_RAW, "inside", ORIENTATIONS[0], (0.8, 0.8, 5.0), seed=5)
TORCH_LABEL_CASE = make_case(RAWS[1], "faces", ORIENTATIONS[0], (0.68, 0.68, 5.0))
TORCH_IMAGE_CASES = [CASES[0], CASES[4], CASES[16],make_case((40, 33, 21), "inside", ORIENTATIONS[9], (0.8, 0.8, 5.0), seed=3),
                     make_case(RAWS[1], "small", ORIENTATIONS[29], SPACINGS[1], pad_to=(10, 10, 10)), TORCH_LABEL_CASE]


def case_inputs(case):
    """(image, label, orientation keywords of amos_prefix) of a case."""
    image, label = raw_volume(case["raw"], case["kind"], case["seed"])
    if case["route"] == "affine":
        how = {"affine": affine_of(case["perm"], case["sign"], case["spacing"])}
    else:
        how = {"spacing": source_spacing(case["perm"], case["spacing"]), "axcodes": axcodes_of(case["perm"], case["sign"])}
    return image, label, how


_REFERENCES = {}


def reference(case):
    key = tuple(sorted((k, v) for k, v in case.items()))
    if key not in _REFERENCES:
        image, label = raw_volume(case["raw"], case["kind"], case["seed"])
        _REFERENCES[key] = forward_chain(image, label, case["perm"], case["sign"], case["spacing"], case["pixdim"], case["pad_to"])
    return _REFERENCES[key]


def run_case(case, device, out=None):
    """amos_prefix of a case on ``device`` -> (image_t, label_t, plan), as tensors."""
    image, label, how = case_inputs(case)
    return amos_prefix(image, label, device, pixdim=case["pixdim"], pad_to=case["pad_to"], out=out, **how)


def check_case(case, device, out=None):
    """The device's result of a case == the yardstick, exactly: plan (box, orientation, extents), image and label."""
    want_i, want_l, stages = reference(case)
    got_i, got_l, plan = run_case(case, device, out)
    lo, hi = stages["box"]
    assert plan.shape == tuple(case["raw"]) and plan.box == (*lo, *hi), (case, plan)
    assert plan.box == (*box_of(case["raw"], case["kind"])[0], *box_of(case["raw"], case["kind"])[1]), (case, plan)
    assert plan.perm == tuple(case["perm"]) and plan.sign == tuple(case["sign"]), (case, plan)
    assert plan.spacing == tuple(case["spacing"]) and plan.pad_front == tuple(w[0] for w in stages["widths"]), (case, plan)
    assert plan.padded_shape == stages["oriented"][0].shape and plan.out_shape == want_i.shape, (case, plan)
    assert got_i.dtype == torch.float32 and got_l.dtype == torch.uint8 and tuple(got_i.shape) == tuple(got_l.shape) == want_i.shape
    assert np.array_equal(got_i.cpu().numpy(), want_i), case
    assert np.array_equal(got_l.cpu().numpy(), want_l), case
    return got_i, got_l, plan


def misaligned_outputs(shape, device):
    """(image, label) tensors of ``shape`` that start 4 bytes (image) and 1 byte (label) past an aligned address: no vector stores."""
    count = int(np.prod(shape))
    buf = torch.full((count + 8,), float("nan"), dtype=torch.float32, device=device)
    shift = 1 + (-(buf.data_ptr() // 4)) % 4
    image = buf[shift:shift + count].view(shape)
    lbuf = torch.full((count + 8,), 255, dtype=torch.uint8, device=device)
    lshift = 1 + (-lbuf.data_ptr()) % 4
    label = lbuf[lshift:lshift + count].view(shape)
    assert image.data_ptr() % 16 == 4 and label.data_ptr() % 4 == 1
    return image, label


def check_restore(case, device, identity):
    """``identity`` (pixdim == spacing): restore_label(label_t) == the raw label inside the box and 0 outside.  Otherwise: restore_label
    of a map of distinct values on the respaced grid == inverse_chain of it; uint8 and int64 predictions agree."""
    image, label = raw_volume(case["raw"], case["kind"], case["seed"])
    _, want_l, stages = reference(case)
    got_i, got_l, plan = run_case(case, device)
    if identity:
        assert plan.spacing == plan.pixdim
        back = restore_label(got_l, plan).cpu().numpy()
        lo, hi = stages["box"]
        want = np.zeros_like(label)
        region = tuple(slice(a, b) for a, b in zip(lo, hi))
        want[region] = label[region]
        assert back.dtype == np.uint8 and np.array_equal(back, want), case
    count = int(np.prod(plan.out_shape))
    pred = (1 + np.arange(count) % 251).astype(np.uint8).reshape(plan.out_shape)          # never 0: the outside of the box is told apart
    want = inverse_chain(pred, plan.shape, stages["box"], case["perm"], case["sign"], case["spacing"], case["pixdim"], stages["widths"])
    back8 = restore_label(torch.from_numpy(pred).to(device), plan).cpu().numpy()
    back64 = restore_label(torch.from_numpy(pred.astype(np.int64)).to(device)[None, None], plan).cpu().numpy()
    assert np.array_equal(back8, want) and np.array_equal(back64, want), case


# ---- the independent cross-check: torch's grid_sample on the CPU ------------------------------------------------------------------------

def torch_reference(case):
    """(image, label, distance) by ``F.grid_sample(align_corners=True, padding_mode="border")`` — bilinear / nearest — on the yardstick's
    windowed, oriented, padded crop, with the grid ``2 x / (m - 1) - 1`` from the fp64 coordinates; an axis of extent 1 gets the
    coordinate 0 (its normalisation would divide by zero).  ``distance``: the smallest distance of any coordinate, on axes of extent > 1,
    to a half-integer (the nearest-neighbour result is only defined away from ties)."""
    import torch.nn.functional as F
    _, _, stages = reference(case)
    xi, xl = stages["oriented"]
    m = xi.shape
    coords, distance = [], np.inf
    for a in range(3):
        x = stages["taps"][a][0]
        if m[a] > 1:
            coords.append(2.0 * x / (m[a] - 1) - 1.0)
            distance = min(distance, float(np.abs((x - np.floor(x)) - 0.5).min()))
        else:
            coords.append(np.zeros_like(x))
    g0, g1, g2 = np.meshgrid(*coords, indexing="ij")
    grid = torch.from_numpy(np.stack([g2, g1, g0], axis=-1).astype(np.float32))[None]   # grid_sample wants (x, y, z) = (axis 2, 1, 0)
    image = F.grid_sample(torch.from_numpy(xi)[None, None], grid, mode="bilinear", padding_mode="border", align_corners=True)[0, 0]
    label = F.grid_sample(torch.from_numpy(xl.astype(np.float32))[None, None], grid, mode="nearest", padding_mode="border",
                          align_corners=True)[0, 0]
    return image.numpy(), label.numpy().astype(np.uint8), distance
