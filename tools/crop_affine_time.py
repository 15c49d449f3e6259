"""The affine stage of the BraTS feed on the MI355X -> profiles/crop_affine.json and profiles/crop_affine.md.

usage (GPU box, from the repository root):
    python tools/crop_affine_time.py [--out profiles/crop_affine]

One batch of 2 samples x 4 channels x 96^3 from two volumes of (4, 240, 240, 155) voxels (uniform values, random labels 0..3, made on the
device), the same crop origins for every variant, k = 0 and no flip (so that the single-channel AMOS kernel, whose chain has no quarter
turn in front of the affine, computes the same patch).  The C ABI is called directly with argument arrays built once.  Method, that of
tools/affine_feed_time.py: every variant writes into ROTATING output sets (SETS pairs of image and label buffers, 42 MB a pair, together
more than the 256 MiB Infinity Cache), the variants are timed INTERLEAVED in one process (round r: A, B, C, ..., A, B, ...), each window =
LAUNCHES back-to-back calls between two device events, the figure = window / LAUNCHES, and median, minimum and maximum over ROUNDS are
recorded after a warm-up of every variant.  Variants:

  channels          icl_crop_rotflip_channels (the plain gather), and `channels_again`, the same call a second time in every round,
                    whose ratio to `channels` is the run-to-run spread of this box;
  affine_flags_off  icl_crop_rotflip_affine with every flag 0: the integer path inside the new kernel; bit-equal to `channels`;
  affine_identity   icl_crop_rotflip_affine, every sample affine with M = I: the arithmetic and the taps on the plain access pattern;
                    bit-equal to `channels`;
  affine            icl_crop_rotflip_affine, every sample with a random rotation (angles in +-0.5 rad per axis);
  affine_scalar     the same call with an image output 4 bytes past a 16-byte boundary: the V = 1 instance of the kernel (an affine sample
                    takes one voxel per thread in both instances, so this shows what the misaligned output costs; bit-equal to `affine`);
  four_single       the yardstick, which the parent commit has: four icl_volume_feed_affine launches, one per channel, on the same data
                    (channel c of a volume is a contiguous [240,240,155] array) with the same M, into [4][2,1,96^3] (the label is written
                    by each of the four); every channel bit-equal to `affine`.

No threshold is asserted: this tool records.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from icl_amd import _lib  # noqa: E402
from icl_amd.dataloaders.amos import affine_matrix  # noqa: E402

SHAPE = (240, 240, 155)
CHANNELS = 4
BATCH = 2
PATCH = (96, 96, 96)
SETS = 8
LAUNCHES = 100
ROUNDS = 15
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)


def window(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches      # microseconds a call


def measure(dev):
    L = _lib.lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    volumes = [torch.rand((CHANNELS,) + SHAPE, device=dev, generator=gen) * 4.0 - 1.0 for _ in range(BATCH)]
    label_volumes = [torch.randint(0, 4, SHAPE, device=dev, generator=gen, dtype=torch.uint8) for _ in range(BATCH)]
    rng = np.random.RandomState(5)
    origins = [[int(rng.randint(0, n - r + 1)) for n, r in zip(SHAPE, PATCH)] for _ in range(BATCH)]
    mats = [tuple(affine_matrix(rng.uniform(-0.5, 0.5, 3), 1.0).reshape(-1)) for _ in range(BATCH)]
    ptrs = ctypes.c_void_p * BATCH
    images, labels = ptrs(*[v.data_ptr() for v in volumes]), ptrs(*[v.data_ptr() for v in label_volumes])
    crops = (ctypes.c_int32 * (11 * BATCH))(*[v for o in origins for v in (*SHAPE, 0, -1, 0, 0, 0, *o)])

    def block(flag, matrices):
        return (ctypes.c_double * (10 * BATCH))(*[float(v) for M in matrices for v in (flag, *M)])

    flags_off, identity, rotated = block(0.0, mats), block(1.0, [IDENTITY] * BATCH), block(1.0, mats)
    # the single-channel launches: channel c of volume b as a volume of its own
    plane = SHAPE[0] * SHAPE[1] * SHAPE[2] * 4
    channel_images = [ptrs(*[v.data_ptr() + c * plane for v in volumes]) for c in range(CHANNELS)]
    ints = (ctypes.c_int32 * (14 * BATCH))(*[v for o in origins for v in (*SHAPE, *o, *PATCH, 0, 0, 0, 0, 0)])
    floats = (ctypes.c_float * (2 * BATCH))(*([1.0, 0.0] * BATCH))

    voxels = PATCH[0] * PATCH[1] * PATCH[2]
    sets = [(torch.empty(BATCH * CHANNELS * voxels + 4, device=dev), torch.empty((CHANNELS, BATCH) + PATCH, dtype=torch.int64, device=dev))
            for _ in range(SETS)]
    assert all(i.data_ptr() % 16 == 0 for i, _ in sets)
    turn = {"n": 0}

    def outs(shift=0):
        turn["n"] = (turn["n"] + 1) % SETS
        i, l = sets[turn["n"]]
        return i.data_ptr() + 4 * shift, l.data_ptr()

    def channels():
        _lib.check(L.icl_crop_rotflip_channels(images, labels, crops, BATCH, CHANNELS, *outs(), *PATCH, stream), "crop_rotflip_channels")

    def affine(params, shift=0):
        _lib.check(L.icl_crop_rotflip_affine(images, labels, crops, params, BATCH, CHANNELS, *outs(shift), *PATCH, stream), "crop_rotflip_affine")

    def four_single():
        i, l = outs()
        for c in range(CHANNELS):
            _lib.check(L.icl_volume_feed_affine(channel_images[c], labels, ints, floats, rotated, BATCH, i + 4 * c * BATCH * voxels,
                                                l + 8 * c * BATCH * voxels, *PATCH, stream), "volume_feed_affine")

    variants = {"channels": channels, "channels_again": channels, "affine_flags_off": lambda: affine(flags_off),
                "affine_identity": lambda: affine(identity), "affine": lambda: affine(rotated), "affine_scalar": lambda: affine(rotated, 1),
                "four_single": four_single}

    def result(fn, shift=0):
        """image [B, C, *patch] (four_single: [C, B, *patch]) and label [B, *patch] of one call, copied out of set 0"""
        turn["n"] = SETS - 1                         # the next call writes set 0
        fn()
        torch.cuda.synchronize()
        i, l = sets[0]
        return i[shift:shift + BATCH * CHANNELS * voxels].clone().view(torch.int32), l[0].clone()

    plain = result(channels)
    equal = {}
    for key in ("affine_flags_off", "affine_identity"):
        got = result(variants[key])
        equal[key + "_equals_channels"] = bool(torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1]))
    quad, scalar, single = result(variants["affine"]), result(variants["affine_scalar"], 1), result(four_single)
    equal["affine_scalar_equals_affine"] = bool(torch.equal(quad[0], scalar[0]) and torch.equal(quad[1], scalar[1]))
    by_channel = single[0].view(CHANNELS, BATCH, voxels).transpose(0, 1).contiguous().view(-1)
    equal["four_single_equals_affine"] = bool(torch.equal(quad[0], by_channel) and torch.equal(quad[1], single[1]))
    equal["affine_differs_from_channels"] = not torch.equal(quad[0], plain[0])

    for fn in variants.values():                     # warm-up: code objects loaded, every buffer touched
        window(fn, 2 * SETS)
    times = {k: [] for k in variants}
    for _ in range(ROUNDS):
        for k, fn in variants.items():
            times[k].append(window(fn, LAUNCHES))
    med = {k: statistics.median(v) for k, v in times.items()}
    written = BATCH * voxels * (4 * CHANNELS + 8)
    return {"source": [CHANNELS, *SHAPE], "batch": BATCH, "patch": list(PATCH), "origins": origins, "bytes_written": written,
            "us_per_call": {k: {"median": round(med[k], 2), "min": round(min(v), 2), "max": round(max(v), 2)} for k, v in times.items()},
            "spread_channels_again_over_channels": round(med["channels_again"] / med["channels"], 4),
            "flags_off_over_channels": round(med["affine_flags_off"] / med["channels"], 4),
            "identity_over_channels": round(med["affine_identity"] / med["channels"], 3),
            "affine_over_channels": round(med["affine"] / med["channels"], 3),
            "affine_scalar_over_affine": round(med["affine_scalar"] / med["affine"], 3),
            "affine_over_four_single": round(med["affine"] / med["four_single"], 3),
            "affine_written_gb_per_s": round(written / med["affine"] / 1e3, 1), "equal": equal}


def markdown(res):
    r = res["result"]
    lines = ["# The affine stage of the BraTS feed (`crop_rotflip_affine_kernel` in `datafeed.h`)", "",
             f"Written by `tools/crop_affine_time.py` on one {res['device']}; the raw figures are in `crop_affine.json`, the method and the variants",
             f"in the tool's docstring: one batch of {r['batch']} × {r['source'][0]} × 96³ from (4, 240, 240, 155) volumes, outputs rotating through "
             f"{res['sets']} buffer sets,", f"variants interleaved in one process, {res['rounds']} rounds of {res['launches_per_window']} back-to-back "
             "calls between two device events after a warm-up.", "", "| per call | median µs | min | max |", "|---|---|---|---|"]
    for k, t in r["us_per_call"].items():
        lines.append(f"| `{k}` | {t['median']} | {t['min']} | {t['max']} |")
    lines += ["", f"* spread of the box, `channels_again / channels`: {r['spread_channels_again_over_channels']}.",
              f"* all flags 0 / `channels`: {r['flags_off_over_channels']} (bit-equal: {r['equal']['affine_flags_off_equals_channels']}); "
              f"M = I / `channels`: {r['identity_over_channels']} (bit-equal: {r['equal']['affine_identity_equals_channels']}).",
              f"* rotated / `channels`: {r['affine_over_channels']}; the rotated gather writes {r['affine_written_gb_per_s']} GB/s.",
              f"* **one launch / four single-channel launches (`affine / four_single`): {r['affine_over_four_single']}** "
              f"(every channel and the label bit-equal: {r['equal']['four_single_equals_affine']}).",
              f"* misaligned image output, the `V = 1` instance, on the same work (`affine_scalar / affine`): {r['affine_scalar_over_affine']} "
              f"(bit-equal: {r['equal']['affine_scalar_equals_affine']}).", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crop_affine"), help="path without extension: .json and .md are written")
    ap.add_argument("--notes", default=os.path.join(ROOT, "profiles", "crop_affine_notes.md"),
                    help="a markdown file whose text is appended to the .md when it exists (registers, what bounds the kernel, open work)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("crop_affine_time.py needs a HIP device")
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "sets": SETS, "launches_per_window": LAUNCHES, "rounds": ROUNDS, "result": measure(dev)}
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
    bad = [k for k, v in res["result"]["equal"].items() if not v]
    if bad:
        raise SystemExit(f"results differ: {bad}")


if __name__ == "__main__":
    main()
