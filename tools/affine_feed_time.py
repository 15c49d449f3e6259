"""The affine stage of the 3-D feed on the MI355X -> profiles/affine_feed.json and profiles/affine_feed.md.

usage (GPU box, from the repository root):
    python tools/affine_feed_time.py [--parent PATH/libicl_hip.so] [--out profiles/affine_feed]

One batch of 8 x 96^3 from four volumes of (130, 101, 70), (96, 96, 96), (97, 140, 96), (60, 200, 111) voxels (hash-filled image, a few
balls of labels), two crops a volume, the same crops, flips, quarter turns and intensities for every variant.  The C ABI is called
directly with argument arrays built once.  Method: every variant writes into ROTATING output sets (SETS pairs of image and label
buffers, 85 MB a pair, together more than the 256 MiB Infinity Cache, so a call never rewrites lines its predecessor left in cache);
the variants are timed INTERLEAVED in one process (round r: A, B, C, ..., A, B, ...), each window = LAUNCHES back-to-back calls between
two device events, the figure = window / LAUNCHES, and median, minimum and maximum over ROUNDS are recorded after a warm-up of every
variant.  The 22 MB of source volumes stay cache-resident in every variant alike.  Three measurements:

  regression   icl_volume_feed of this build (`plain`, and `plain_again`: the same call a second time in every round, whose ratio to
               `plain` is the run-to-run spread of this box) against the same entry point of the build of the parent commit
               (`plain_parent`, only with --parent: the other library is loaded side by side with ctypes), at 96^3 (the quad
               kernel) and at 96 x 96 x 90 (the one-voxel kernel).  Outputs compared bit for bit.  With --stages-out, the same
               check for the other six gather entries: icl_volume_feed_origins, icl_volume_feed_affine with all flags 1 and with
               all flags 0, icl_volume_feed_affine_origins, icl_crop_rotflip, icl_crop_rotflip_channels at C = 4 and
               icl_crop_rotflip_affine at C = 4 with all flags 1 and with all flags 0, each with its own `_again` and `_parent`; the band for this / parent is 1 +- twice the largest |again / first - 1| of the run
               (the ratio of two independent medians carries the spread of both); written to <stages-out>.json.
  affine       icl_volume_feed_affine with every sample affine (angles in +-0.5 rad, anisotropic zoom in 0.7 .. 1.4) and with every
               flag 0 (the integer path inside the new kernel), against `plain`, and as a fraction of the device copy rate for the
               bytes written (`copy`: Tensor.copy_ of one image and one label buffer, device to device); `affine_identity`: every
               sample affine with M = I, the same arithmetic and tap count on the access pattern of the plain feed, which separates
               what the rotated gather costs from what the arithmetic and the taps cost.
  context      scipy.ndimage.affine_transform of one 96^3 patch on the host (order 1 image, order 0 label), one core.

No threshold is asserted: this tool records.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from icl_amd import _lib  # noqa: E402
from icl_amd.dataloaders.amos import affine_matrix, amos_volume_store  # noqa: E402
from icl_amd.dataloaders.brats2019 import DeviceVolumeStore, draw_rotflip_crop  # noqa: E402
from icl_amd.utils.hashfill import hash_uniform_np  # noqa: E402

SHAPES = [(130, 101, 70), (96, 96, 96), (97, 140, 96), (60, 200, 111)]
PER_VOLUME = 2
SETS = 4
LAUNCHES = 100
ROUNDS = 15


def make_volume(j, shape):
    image = hash_uniform_np(int(np.prod(shape)), 300 + j, 1.0).astype(np.float32).reshape(shape)
    label = np.zeros(shape, dtype=np.uint8)
    rng = np.random.RandomState(17 + j)
    grid = np.indices(shape)
    for organ in range(1, 6):
        centre = [int(rng.randint(0, n)) for n in shape]
        radius = int(rng.randint(4, 10))
        label[sum((grid[a] - centre[a]) ** 2 for a in range(3)) <= radius * radius] = organ
    return image, label


def window(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches      # microseconds a call


GATHER_ENTRIES = ("icl_volume_feed", "icl_volume_feed_origins", "icl_volume_feed_affine", "icl_volume_feed_affine_origins",
                  "icl_crop_rotflip", "icl_crop_rotflip_channels", "icl_crop_rotflip_affine")


def load_parent(path):
    """The parent commit's library beside this build's: the seven gather entries, with the signatures of icl_amd/_lib.py (the ABI is shared)."""
    lib = ctypes.CDLL(path)
    for name in GATHER_ENTRIES:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib._SIGNATURES[name]
    return lib


def measure_entries(L, parent, store, store4, dev, roi):
    """The regression check of the six gather entries beside icl_volume_feed, on the batch of ``measure``: every entry of this build
    (`x`, and `x_again` in the same round), against the parent's (`x_parent`), interleaved, outputs rotating and compared bit for bit."""
    vols, rows, mats = make_rows(roi)
    m = len(vols)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ptrs = ctypes.c_void_p * m
    images, labels = ptrs(*[store.images[j].data_ptr() for j in vols]), ptrs(*[store.labels[j].data_ptr() for j in vols])
    images4 = ptrs(*[store4.images[j].data_ptr() for j in vols])
    ints = (ctypes.c_int32 * (14 * m))(*[int(v) for r in rows for v in r[:14]])
    floats = (ctypes.c_float * (2 * m))(*[float(v) for r in rows for v in r[14:16]])
    affine_on = (ctypes.c_double * (10 * m))(*[float(v) for M in mats for v in (1.0, *M)])
    affine_off = (ctypes.c_double * (10 * m))(*[float(v) for M in mats for v in (0.0, *M)])
    origins = torch.tensor([r[3:6] for r in rows], dtype=torch.int32, device=dev)
    np.random.seed(23)
    crops = (ctypes.c_int32 * (11 * m))(*[int(v) for j in vols for v in draw_rotflip_crop(SHAPES[j], roi)])
    channels = int(store4.channels)
    sets = {c: [(torch.empty((m, c) + roi, device=dev), torch.empty((m,) + roi, dtype=torch.int64, device=dev)) for _ in range(SETS)]
            for c in (1, channels)}
    turn = {"n": 0}

    def outs(c=1):
        turn["n"] = (turn["n"] + 1) % SETS
        i, l = sets[c][turn["n"]]
        return i.data_ptr(), l.data_ptr()

    calls = {
        "volume_feed_origins": lambda lib: lib.icl_volume_feed_origins(images, labels, ints, floats, m, origins.data_ptr(), *outs(), *roi, stream),
        "volume_feed_affine": lambda lib: lib.icl_volume_feed_affine(images, labels, ints, floats, affine_on, m, *outs(), *roi, stream),
        "volume_feed_affine_flags_off": lambda lib: lib.icl_volume_feed_affine(images, labels, ints, floats, affine_off, m, *outs(), *roi, stream),
        "volume_feed_affine_origins": lambda lib: lib.icl_volume_feed_affine_origins(images, labels, ints, floats, affine_on, m,
                                                                                     origins.data_ptr(), *outs(), *roi, stream),
        "crop_rotflip": lambda lib: lib.icl_crop_rotflip(images, labels, crops, m, *outs(), *roi, stream),
        "crop_rotflip_channels": lambda lib: lib.icl_crop_rotflip_channels(images4, labels, crops, m, channels, *outs(channels), *roi, stream),
        "crop_rotflip_affine": lambda lib: lib.icl_crop_rotflip_affine(images4, labels, crops, affine_on, m, channels, *outs(channels), *roi, stream),
        "crop_rotflip_affine_flags_off": lambda lib: lib.icl_crop_rotflip_affine(images4, labels, crops, affine_off, m, channels, *outs(channels),
                                                                                 *roi, stream),
    }
    multi = ("crop_rotflip_channels", "crop_rotflip_affine", "crop_rotflip_affine_flags_off")      # the entries that write C channels

    def run(name, lib):
        if calls[name](lib) != 0:
            raise SystemExit(f"{name} failed: {L.icl_last_error()}")

    def result(name, lib):
        c = channels if name in multi else 1
        turn["n"] = SETS - 1                         # the next call writes set 0
        run(name, lib)
        torch.cuda.synchronize()
        return sets[c][0][0].view(torch.int32).clone(), sets[c][0][1].clone()

    equal, variants = {}, {}
    for name in calls:
        ours, theirs = result(name, L), result(name, parent)
        equal[name] = bool(torch.equal(ours[0], theirs[0]) and torch.equal(ours[1], theirs[1]))
        del ours, theirs
        for suffix, lib in (("", L), ("_again", L), ("_parent", parent)):
            variants[name + suffix] = (lambda name=name, lib=lib: run(name, lib))
    for fn in variants.values():                     # warm-up: code objects loaded, every buffer touched
        window(fn, 2 * SETS)
    times = {k: [] for k in variants}
    for _ in range(ROUNDS):
        for k, fn in variants.items():
            times[k].append(window(fn, LAUNCHES))
    med = {k: statistics.median(v) for k, v in times.items()}
    return {"roi": list(roi), "batch": m, "channels_of_crop_rotflip_channels": channels, "channels_of_crop_rotflip_affine": channels,
            "us_per_call": {k: {"median": round(med[k], 2), "min": round(min(v), 2), "max": round(max(v), 2)} for k, v in times.items()},
            "again_over_first": {k: round(med[k + "_again"] / med[k], 4) for k in calls},
            "now_over_parent": {k: round(med[k] / med[k + "_parent"], 4) for k in calls}, "equal": equal}


def stages_record(device, blocks):
    """profiles/feed_stages.json: per ROI the figures of ``measure`` (icl_volume_feed) and ``measure_entries``, the spread of the run
    (the largest |again / first - 1| over every entry and ROI) and the band 1 +- twice that for median(this) / median(parent)."""
    spread, entries = 0.0, []
    for key, (plain, others) in blocks.items():
        spread = max([spread, abs(plain["spread_plain_again_over_plain"] - 1)] + [abs(v - 1) for v in others["again_over_first"].values()])
        entries.append((key, "volume_feed", plain["us_per_call"]["plain"]["median"], plain["us_per_call"]["plain_parent"]["median"],
                        plain["spread_plain_again_over_plain"], plain["now_over_parent"], plain["equal"]["plain_parent"]))
        for name in others["now_over_parent"]:
            t = others["us_per_call"]
            entries.append((key, name, t[name]["median"], t[name + "_parent"]["median"], others["again_over_first"][name],
                            others["now_over_parent"][name], others["equal"][name]))
    lo, hi = 1 - 2 * spread, 1 + 2 * spread
    table = [{"roi": key, "entry": name, "median_us": now, "parent_median_us": par, "again_over_first": again, "now_over_parent": ratio,
              "bit_equal_to_parent": eq, "verdict": "slower than the band" if ratio > hi else "faster than the band" if ratio < lo else "inside the band"}
             for key, name, now, par, again, ratio, eq in entries]
    return {"device": device, "sets": SETS, "launches_per_window": LAUNCHES, "rounds": ROUNDS, "spread": round(spread, 4),
            "band": [round(lo, 4), round(hi, 4)], "entries": table,
            "raw": {key: {"volume_feed": plain, "other_entries": others} for key, (plain, others) in blocks.items()}}


def stages_markdown(rec):
    lines = [f"Measured by `tools/affine_feed_time.py --parent ... --stages-out ...` on one {rec['device']}: {rec['rounds']} rounds of "
             f"{rec['launches_per_window']} back-to-back calls per variant, variants interleaved, outputs rotating through {rec['sets']} sets.",
             f"Spread of the run (largest |again / first - 1|): {rec['spread']}; band for now / parent: {rec['band'][0]} .. {rec['band'][1]}.", "",
             "| ROI | entry | median µs | parent median µs | again / first | now / parent | bit-equal to parent | verdict |",
             "|---|---|---|---|---|---|---|---|"]
    for e in rec["entries"]:
        lines.append(f"| {e['roi']} | `{e['entry']}` | {e['median_us']} | {e['parent_median_us']} | {e['again_over_first']} | "
                     f"{e['now_over_parent']} | {e['bit_equal_to_parent']} | {e['verdict']} |")
    return "\n".join(lines) + "\n"


def make_rows(roi):
    """8 feed rows (origins inside their ranges, all flips and quarter turns over the batch) and 8 matrices."""
    rng = np.random.RandomState(5)
    vols = [j for j in range(len(SHAPES)) for _ in range(PER_VOLUME)]
    rows, mats = [], []
    for q, j in enumerate(vols):
        n = SHAPES[j]
        size = [min(r, e) for r, e in zip(roi, n)]
        left = [(r - s) // 2 for r, s in zip(roi, size)]
        origin = [int(rng.randint(0, e - s + 1)) for e, s in zip(n, size)]
        k = q % 4 if roi[0] == roi[1] else 2 * (q % 2)
        rows.append([*n, *origin, *size, *left, q % 8, k, 1.0 + 0.0625 * (q % 3), 0.03125 * (q % 2)])
        mats.append(affine_matrix(rng.uniform(-0.5, 0.5, 3), rng.uniform(0.7, 1.4, 3)).reshape(-1))
    return vols, rows, mats


def measure(L, parent, store, dev, roi, with_affine):
    vols, rows, mats = make_rows(roi)
    m = len(vols)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ptrs = ctypes.c_void_p * m
    images, labels = ptrs(*[store.images[j].data_ptr() for j in vols]), ptrs(*[store.labels[j].data_ptr() for j in vols])
    ints = (ctypes.c_int32 * (14 * m))(*[int(v) for r in rows for v in r[:14]])
    floats = (ctypes.c_float * (2 * m))(*[float(v) for r in rows for v in r[14:16]])
    affine_on = (ctypes.c_double * (10 * m))(*[float(v) for M in mats for v in (1.0, *M)])
    affine_off = (ctypes.c_double * (10 * m))(*[float(v) for M in mats for v in (0.0, *M)])
    affine_eye = (ctypes.c_double * (10 * m))(*[float(v) for _ in mats for v in (1.0, 1, 0, 0, 0, 1, 0, 0, 0, 1)])
    sets = [(torch.empty((m, 1) + roi, device=dev), torch.empty((m,) + roi, dtype=torch.int64, device=dev)) for _ in range(SETS)]
    turn = {"n": 0}

    def outputs():
        turn["n"] = (turn["n"] + 1) % SETS
        return sets[turn["n"]]

    def plain(lib=L):
        i, l = outputs()
        rc = lib.icl_volume_feed(images, labels, ints, floats, m, i.data_ptr(), l.data_ptr(), *roi, stream)
        if rc != 0:
            raise SystemExit(f"icl_volume_feed failed ({rc})")

    def affine(block=affine_on):
        i, l = outputs()
        _lib.check(L.icl_volume_feed_affine(images, labels, ints, floats, block, m, i.data_ptr(), l.data_ptr(), *roi, stream), "volume_feed_affine")

    def copy():
        i, l = outputs()
        i.copy_(sets[0][0] if i is not sets[0][0] else sets[1][0])
        l.copy_(sets[0][1] if l is not sets[0][1] else sets[1][1])

    variants = {"plain": plain, "plain_again": plain}
    if parent is not None:
        variants["plain_parent"] = lambda: plain(parent)
    if with_affine:
        variants.update({"affine_all_flags_off": lambda: affine(affine_off), "affine_identity": lambda: affine(affine_eye), "affine": affine,
                         "copy": copy})

    # results once, into buffers of their own, for the bit comparisons
    def result(fn):
        turn["n"] = SETS - 1                         # the next call writes set 0
        fn()
        torch.cuda.synchronize()
        return sets[0][0].clone(), sets[0][1].clone()

    ref_image, ref_label = result(plain)
    equal = {}
    for key in ("plain_parent", "affine_all_flags_off", "affine_identity"):
        if key in variants:
            gi, gl = result(variants[key])
            equal[key] = bool(torch.equal(gi.view(torch.int32), ref_image.view(torch.int32)) and torch.equal(gl, ref_label))
    if with_affine:
        a1, a2 = result(affine), result(affine)
        equal["affine_repeats"] = bool(torch.equal(a1[0].view(torch.int32), a2[0].view(torch.int32)) and torch.equal(a1[1], a2[1]))

    for fn in variants.values():                     # warm-up: code objects loaded, every buffer touched
        window(fn, 2 * SETS)
    times = {k: [] for k in variants}
    for _ in range(ROUNDS):
        for k, fn in variants.items():
            times[k].append(window(fn, LAUNCHES))
    med = {k: statistics.median(v) for k, v in times.items()}
    voxels = m * roi[0] * roi[1] * roi[2]
    out = {"roi": list(roi), "batch": m, "bytes_written": 12 * voxels,
           "us_per_call": {k: {"median": round(med[k], 2), "min": round(min(v), 2), "max": round(max(v), 2)} for k, v in times.items()},
           "spread_plain_again_over_plain": round(med["plain_again"] / med["plain"], 4),
           "spread_plain_max_over_min": round(max(times["plain"]) / min(times["plain"]), 4), "equal": equal}
    if parent is not None:
        out["now_over_parent"] = round(med["plain"] / med["plain_parent"], 4)
    if with_affine:
        out["affine_over_plain"] = round(med["affine"] / med["plain"], 3)
        out["flags_off_over_plain"] = round(med["affine_all_flags_off"] / med["plain"], 4)
        out["identity_over_plain"] = round(med["affine_identity"] / med["plain"], 3)
        out["written_gb_per_s"] = {k: round(12 * voxels / med[k] / 1e3, 1) for k in ("plain", "affine", "copy")}
        out["affine_fraction_of_copy_rate"] = round(med["copy"] / med["affine"], 3)
        out["affine_ns_per_voxel_chipwide"] = round(med["affine"] * 1e3 / voxels, 5)
    return out, rows, mats


def scipy_context(rows, mats, roi):
    """The same transform of the first sample with scipy on the host: seconds for the image (order 1) and the label (order 0)."""
    from scipy import ndimage
    image, label = make_volume(0, SHAPES[0])
    row, M = rows[0], np.asarray(mats[0]).reshape(3, 3)
    ctr = (np.asarray(roi, dtype=np.float64) - 1) / 2
    offset = np.asarray(row[3:6], dtype=np.float64) - np.asarray(row[9:12], dtype=np.float64) + ctr - M @ ctr
    t_image, t_label = [], []
    for _ in range(3):
        t0 = time.perf_counter()
        ndimage.affine_transform(image, M, offset=offset, output_shape=roi, order=1, mode="grid-constant", cval=0.0)
        t1 = time.perf_counter()
        ndimage.affine_transform(label, M, offset=offset, output_shape=roi, order=0, mode="grid-constant", cval=0)
        t2 = time.perf_counter()
        t_image.append(t1 - t0)
        t_label.append(t2 - t1)
    return {"image_order1_ms": round(1e3 * statistics.median(t_image), 1), "label_order0_ms": round(1e3 * statistics.median(t_label), 1)}


def markdown(res):
    big, odd, ctx = res["roi_96"], res["roi_90"], res["scipy_one_patch"]

    def table(block, keys):
        lines = ["| per call | median µs | min | max |", "|---|---|---|---|"]
        for k in keys:
            if k in block["us_per_call"]:
                t = block["us_per_call"][k]
                lines.append(f"| `{k}` | {t['median']} | {t['min']} | {t['max']} |")
        return "\n".join(lines)

    parent = "now / parent" in res["columns"]
    text = [
        "# The affine stage of the 3-D feed (`volume_feed_affine_kernel` in `datafeed.h`)",
        "",
        f"Written by `tools/affine_feed_time.py` on one {res['device']}; the raw figures are in `affine_feed.json`, the method in the tool's",
        f"docstring: one batch of 8 × 96³, outputs rotating through {res['sets']} buffer sets (85 MB each), variants interleaved in one process,",
        f"{res['rounds']} rounds of {res['launches_per_window']} back-to-back calls between two device events after a warm-up.",
        "",
        "## 1. Regression check: `icl_volume_feed` against the parent commit's build",
        "",
        "`plain` and `plain_again` are the same call of this build, timed twice in every round: their ratio is the spread of this box.",
        ("`plain_parent` is the parent commit's library, loaded side by side." if parent else
         "No parent library was given (`--parent`): the comparison with the parent commit's build was NOT measured in this run."),
        "",
        "96 × 96 × 96 (`volume_feed_kernel<4, false>`):",
        "",
        table(big, ("plain", "plain_again", "plain_parent")),
        "",
        "96 × 96 × 90 (`volume_feed_kernel<1, false>`):",
        "",
        table(odd, ("plain", "plain_again", "plain_parent")),
        "",
        f"* spread, `plain_again / plain`: {big['spread_plain_again_over_plain']} (96³), {odd['spread_plain_again_over_plain']} (96 × 96 × 90); "
        f"max / min of `plain` over the rounds: {big['spread_plain_max_over_min']}, {odd['spread_plain_max_over_min']}.",
    ]
    if parent:
        text += [f"* **now / parent: {big['now_over_parent']} (96³), {odd['now_over_parent']} (96 × 96 × 90)**; outputs bit-equal: "
                 f"{big['equal'].get('plain_parent')}, {odd['equal'].get('plain_parent')}."]
    text += [
        "",
        "## 2. The affine gather",
        "",
        "Every sample affine (angles in ±0.5 rad, anisotropic zoom in 0.7 … 1.4), and every flag 0 (the integer path inside the new kernel),",
        "against `plain`; `copy` is `Tensor.copy_` of one image and one label buffer (the 85 MB a call writes, read from another set).",
        "",
        table(big, ("plain", "affine_all_flags_off", "affine_identity", "affine", "copy")),
        "",
        f"* **affine / plain: {big['affine_over_plain']}**; all flags off / plain: {big['flags_off_over_plain']} "
        f"(bit-equal to `plain`: {big['equal'].get('affine_all_flags_off')}); two affine runs bit-equal: {big['equal'].get('affine_repeats')}.",
        f"* `affine_identity` (every sample affine, M = I: the same arithmetic and taps on the plain feed's access pattern) / plain: "
        f"{big['identity_over_plain']} (bit-equal to `plain`: {big['equal'].get('affine_identity')}).",
        f"* bytes written per second: plain {big['written_gb_per_s']['plain']} GB/s, affine {big['written_gb_per_s']['affine']} GB/s, "
        f"copy {big['written_gb_per_s']['copy']} GB/s: **the affine gather writes at {big['affine_fraction_of_copy_rate']} of the device copy's rate**.",
        "",
        "## 3. Context: the same transform on the host",
        "",
        f"`scipy.ndimage.affine_transform` of one 96³ patch (sample 0), one core: image (order 1) {ctx['image_order1_ms']} ms, label (order 0) "
        f"{ctx['label_order0_ms']} ms.  The device call above transforms eight such patches, image and label.",
        "",
    ]
    return "\n".join(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="libicl_hip.so of the parent commit's build, for the regression check")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "affine_feed"), help="path without extension: .json and .md are written")
    ap.add_argument("--notes", default=os.path.join(ROOT, "profiles", "affine_feed_notes.md"),
                    help="a markdown file whose text is appended to the .md when it exists (what bounds the kernel, open work)")
    ap.add_argument("--stages-out", default=None, help="with --parent: path without extension of the record of all seven gather entries "
                    "against the parent's (.json is written, its table is printed), e.g. profiles/feed_stages")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("affine_feed_time.py needs a HIP device")
    dev = torch.device("cuda", 0)
    L = _lib.lib()
    parent = load_parent(a.parent) if a.parent else None
    store = amos_volume_store([make_volume(j, s) for j, s in enumerate(SHAPES)], dev)
    big, rows, mats = measure(L, parent, store, dev, (96, 96, 96), True)
    odd, _, _ = measure(L, parent, store, dev, (96, 96, 90), False)
    if parent is not None and a.stages_out:
        store4 = DeviceVolumeStore([(np.stack([make_volume(j + 10 * c, s)[0] for c in range(4)]), make_volume(j, s)[1])
                                    for j, s in enumerate(SHAPES)], dev)
        rec = stages_record(torch.cuda.get_device_name(0), {"96 x 96 x 96": (big, measure_entries(L, parent, store, store4, dev, (96, 96, 96))),
                                                            "96 x 96 x 90": (odd, measure_entries(L, parent, store, store4, dev, (96, 96, 90)))})
        with open(a.stages_out + ".json", "w") as f:
            json.dump(rec, f, indent=1)
        print(stages_markdown(rec), flush=True)
        bad = [f"{e['entry']} at {e['roi']}" for e in rec["entries"] if not e["bit_equal_to_parent"]]
        if bad:
            raise SystemExit(f"results differ from the parent's: {bad}")
    res = {"device": torch.cuda.get_device_name(0), "extents": [list(s) for s in SHAPES], "sets": SETS, "launches_per_window": LAUNCHES,
           "rounds": ROUNDS, "columns": ["now / parent"] if parent is not None else [], "roi_96": big, "roi_90": odd,
           "scipy_one_patch": scipy_context(rows, mats, (96, 96, 96))}
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out + ".json", "w") as f:
        json.dump(res, f, indent=1)
    text = markdown(res)
    if a.notes and os.path.exists(a.notes):
        text += "\n" + open(a.notes).read()
    with open(a.out + ".md", "w") as f:
        f.write(text)
    print("wrote", a.out + ".json", a.out + ".md")
    bad = [k for block in (big, odd) for k, v in block["equal"].items() if not v]
    if bad:
        raise SystemExit(f"results differ: {bad}")


if __name__ == "__main__":
    main()
