"""The pos/neg feed against the feed with host origins on the MI355X -> profiles/posneg_feed_time.json.

usage (GPU box, from the repository root):  python tools/posneg_feed_time.py [--out profiles/posneg_feed_time.json]

One batch of 8 x 96^3 from four volumes of (130, 101, 70), (96, 96, 96), (97, 140, 96), (60, 200, 111) voxels (hash-filled image, a few
balls of labels: sparse foreground), two crops a volume, the same crops for every variant.  The C ABI is called directly with argument
arrays built once, so the host's share of a call is the ctypes call and the launch, not the marshalling.  Variants, timed interleaved in
ONE process (round r: A, B, C, D, A, B, ...), each window = LAUNCHES back-to-back calls between two device events, the figure = window /
LAUNCHES, median over ROUNDS after a warm-up of every variant:
  host_origins     icl_volume_feed: the gather with the origins in the argument record (the path before this feed existed)
  device_origins   icl_volume_feed_origins alone: the same gather reading the origins from device memory
  select           icl_rank_select alone: 8 workgroups, one tile (1,024 voxels, 5 B each) and ~10 prefix words a sample
  select_gather    icl_rank_select then icl_volume_feed_origins: what OnDeviceAugmentPosNeg.batch launches per chunk
and, once per volume after a warm-up build, median of BUILDS: index_build (icl_rank_index_build, two launches) with its rate against
the 5 B a voxel it reads.  `equal`: the three gathers wrote the same bits.  The expectation (README "noise": ~1 % drift within a
session, ~3 % between boxes): device_origins / host_origins within 5 % of 1; beyond that `flag` is true and profiles/posneg_feed.md
has to say why.  No threshold is asserted: this tool only records.
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
from icl_amd.dataloaders.amos import KIND_BG, KIND_FG, ForegroundIndex, amos_volume_store, rank_tile  # noqa: E402
from icl_amd.utils.hashfill import hash_uniform_np  # noqa: E402

ROI = (96, 96, 96)
SHAPES = [(130, 101, 70), (96, 96, 96), (97, 140, 96), (60, 200, 111)]
PER_VOLUME = 2
LAUNCHES = 200
ROUNDS = 15
BUILDS = 15


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "posneg_feed_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("posneg_feed_time.py needs a HIP device")
    dev = torch.device("cuda", 0)
    L = _lib.lib()
    store = amos_volume_store([make_volume(j, s) for j, s in enumerate(SHAPES)], dev)
    index = ForegroundIndex(store, 0.0)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    # the batch: per volume one foreground and one background centre, all flips and quarter turns over the batch
    vols = [j for j in range(len(SHAPES)) for _ in range(PER_VOLUME)]
    m = len(vols)
    rows = []
    for q, j in enumerate(vols):
        n = SHAPES[j]
        size = [min(r, e) for r, e in zip(ROI, n)]
        left = [(r - s) // 2 for r, s in zip(ROI, size)]
        kind = KIND_FG if q % 2 == 0 else KIND_BG
        rank = (index.n_fg[j] if kind == KIND_FG else index.n_bg[j]) // 3
        rows.append([*n, 0, 0, 0, *size, *left, q % 8, q % 4, 1.0 + 0.0625 * (q % 3), 0.03125 * (q % 2), kind, rank])
    ptrs = ctypes.c_void_p * m
    images, labels = ptrs(*[store.images[j].data_ptr() for j in vols]), ptrs(*[store.labels[j].data_ptr() for j in vols])
    fgs, bgs = ptrs(*[index.fg[j].data_ptr() for j in vols]), ptrs(*[index.bg[j].data_ptr() for j in vols])
    select = (ctypes.c_int32 * (8 * m))(*[int(v) for r in rows for v in (*r[:3], r[16], r[17], *r[6:9])])
    floats = (ctypes.c_float * (2 * m))(*[float(v) for r in rows for v in r[14:16]])
    origins = torch.zeros((m, 3), dtype=torch.int32, device=dev)
    _lib.check(L.icl_rank_select(images, labels, fgs, bgs, select, 0.0, m, origins.data_ptr(), stream), "rank_select")
    host_origins = origins.cpu().tolist()                       # read back ONCE, before any timing: the rows of the host-origin variant
    ints_dev = (ctypes.c_int32 * (14 * m))(*[int(v) for r in rows for v in r[:14]])
    ints_host = (ctypes.c_int32 * (14 * m))(*[int(v) for r, o in zip(rows, host_origins) for v in (*r[:3], *o, *r[6:14])])
    out = {k: (torch.empty((m, 1) + ROI, device=dev), torch.empty((m,) + ROI, dtype=torch.int64, device=dev))
           for k in ("host_origins", "device_origins", "select_gather")}

    def host_feed():
        i, l = out["host_origins"]
        _lib.check(L.icl_volume_feed(images, labels, ints_host, floats, m, i.data_ptr(), l.data_ptr(), *ROI, stream), "volume_feed")

    def device_feed(key="device_origins"):
        i, l = out[key]
        _lib.check(L.icl_volume_feed_origins(images, labels, ints_dev, floats, m, origins.data_ptr(), i.data_ptr(), l.data_ptr(), *ROI, stream),
                   "volume_feed_origins")

    def select_only():
        _lib.check(L.icl_rank_select(images, labels, fgs, bgs, select, 0.0, m, origins.data_ptr(), stream), "rank_select")

    def select_gather():
        select_only()
        device_feed("select_gather")

    variants = {"host_origins": host_feed, "device_origins": device_feed, "select": select_only, "select_gather": select_gather}
    for fn in variants.values():                                # warm-up: code objects loaded, every shape seen
        window(fn, 20)
    times = {k: [] for k in variants}
    for _ in range(ROUNDS):
        for k, fn in variants.items():
            times[k].append(window(fn, LAUNCHES))
    equal = all(torch.equal(out["host_origins"][0].view(torch.int32), out[k][0].view(torch.int32)) and torch.equal(out["host_origins"][1], out[k][1])
                for k in ("device_origins", "select_gather"))

    builds = []
    for j, shape in enumerate(SHAPES):
        image, label = store.images[j], store.labels[j]
        fg, bg = torch.empty_like(index.fg[j]), torch.empty_like(index.bg[j])

        def build():
            _lib.check(L.icl_rank_index_build(image.data_ptr(), label.data_ptr(), *shape, 0.0, fg.data_ptr(), bg.data_ptr(), stream), "rank_index_build")

        window(build, 5)
        us = statistics.median(window(build, 20) for _ in range(BUILDS))
        voxels = int(np.prod(shape))
        builds.append({"extents": list(shape), "voxels": voxels, "index_bytes": 8 * int(index.fg[j].numel()), "n_fg": index.n_fg[j], "n_bg": index.n_bg[j],
                       "build_us": round(us, 2), "read_gb_per_s": round(5 * voxels / us / 1e3, 1),
                       "same_index": bool(torch.equal(fg, index.fg[j]) and torch.equal(bg, index.bg[j]))})

    med = {k: statistics.median(v) for k, v in times.items()}
    ratio = med["device_origins"] / med["host_origins"]
    voxels_out = m * ROI[0] * ROI[1] * ROI[2]
    res = {"device": torch.cuda.get_device_name(0), "batch": m, "roi": list(ROI), "extents": [list(s) for s in SHAPES],
           "launches_per_window": LAUNCHES, "rounds": ROUNDS, "rank_tile": rank_tile(),
           "us_per_call": {k: {"median": round(med[k], 2), "min": round(min(v), 2), "max": round(max(v), 2)} for k, v in times.items()},
           "gather_gb_per_s": {k: round(17 * voxels_out / med[k] / 1e3, 1) for k in ("host_origins", "device_origins")},
           "device_over_host_origins": round(ratio, 4), "flag": bool(abs(ratio - 1) > 0.05),
           "select_bytes_read": m * (5 * rank_tile() + 4 * 12), "origins": host_origins, "equal": bool(equal), "index_build": builds}
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)
    if not equal or not all(b["same_index"] for b in builds):
        raise SystemExit("the variants' results differ")


if __name__ == "__main__":
    main()
