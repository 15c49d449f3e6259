"""Device (volume_feed_kernel) against host (numpy) AMOS data feed on the MI355X -> profiles/amos_feed_time.json.

usage (GPU box, from the repository root):  python tools/amos_feed_time.py [--out profiles/amos_feed_time.json]

Per batch size (4 and 16 samples -> 96^3; hash-filled volumes with seeded extents around 200 x 160 x 120, one of them with a depth
below 96 so that the padding is exercised):
  device_ms      device events around OnDeviceAugmentAMOS.batch (its host-side draws and the launch included); median of 20 after a warm-up
  host_ms        the random transforms of train_inherent_consistent_unet_3D_AMOS22.py:102-133 restated with numpy (slice, np.pad, np.flip,
                 np.rot90, float32 multiply and add), the collation (np.stack) and the upload of image and label, synchronised, in ONE
                 process on the host clock; median of 20 after a warm-up, same parameters as the device batch
  equal          every timed device batch == the host batch, bit for bit
The host figure is numpy itself, not MONAI (not installed here: parity with MONAI's own code is unpinned) and not six loader threads;
divide by the workers you would give it.  No threshold is asserted: this tool only records.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from icl_amd.dataloaders.amos import OnDeviceAugmentAMOS, amos_volume_store  # noqa: E402
from icl_amd.utils.hashfill import hash_uniform_np  # noqa: E402

ROI = (96, 96, 96)
VOLUMES = 16
WARMUP = 5
TIMED = 20


def make_volumes(seed=2022):
    rng = np.random.RandomState(seed)
    volumes = []
    for i in range(VOLUMES):
        shape = (int(rng.randint(170, 231)), int(rng.randint(130, 191)), int(rng.randint(97, 141)))
        if i == 3:
            shape = shape[:2] + (int(rng.randint(70, 96)),)            # depth below the ROI: padded
        n = shape[0] * shape[1] * shape[2]
        image = hash_uniform_np(n, 500 + i, 1.0).reshape(shape)
        label = np.clip(((hash_uniform_np(n, 600 + i, 0.5) + 0.5) * 16).astype(np.int64), 0, 15).astype(np.uint8).reshape(shape)
        volumes.append((image, label))
    return volumes


def host_sample(image, label, row):
    c, s, left, flip, k = row[3:6], row[6:9], row[9:12], row[12], row[13]
    mul, add = np.float32(row[14]), np.float32(row[15])
    window = tuple(slice(c[a], c[a] + s[a]) for a in range(3))
    widths = [(left[a], ROI[a] - s[a] - left[a]) for a in range(3)]
    out = []
    for x in (image, label):
        x = np.pad(x[window], widths, mode="constant", constant_values=0)
        for a in range(3):
            if flip >> a & 1:
                x = np.flip(x, a)
        out.append(np.rot90(x, k, axes=(0, 1)))
    x = out[0] * mul
    x = x + add
    return x[None], out[1].astype(np.int64)[None]


def host_batch(volumes, indices, rows, dev):
    samples = [host_sample(*volumes[i], row) for i, row in zip(indices, rows)]
    image = torch.from_numpy(np.stack([s[0] for s in samples])).to(dev)
    label = torch.from_numpy(np.stack([s[1] for s in samples])).to(dev)
    torch.cuda.synchronize()
    return image, label


def time_batch(volumes, feed, batch, dev):
    rng = np.random.RandomState(7)
    host, device, equal = [], [], True
    for n in range(WARMUP + TIMED):
        indices = [int(v) for v in rng.permutation(VOLUMES)[:batch]]
        if n == WARMUP and 3 not in indices:
            indices[0] = 3                                              # the short volume is in a timed batch
        state = feed.rng.get_state()
        rows = feed.draw(indices)
        feed.rng.set_state(state)                                       # the device call below draws the same rows again
        t0 = time.perf_counter()
        want_image, want_label = host_batch(volumes, indices, rows, dev)
        t_host = (time.perf_counter() - t0) * 1e3
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        got = feed.batch(indices)
        e1.record()
        torch.cuda.synchronize()
        if n >= WARMUP:
            host.append(t_host)
            device.append(e0.elapsed_time(e1))
            equal = equal and torch.equal(got["image"], want_image) and torch.equal(got["label"], want_label)
    return {"batch": batch, "roi": list(ROI), "timed": TIMED, "warmup": WARMUP,
            "device_ms": round(statistics.median(device), 4), "device_ms_min": round(min(device), 4),
            "host_ms": round(statistics.median(host), 3), "host_ms_min": round(min(host), 3), "equal": bool(equal)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "amos_feed_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("amos_feed_time.py needs a HIP device")
    dev = torch.device("cuda", 0)
    volumes = make_volumes()
    store = amos_volume_store(volumes, dev)
    # probabilities of the trainer, except that flips and rotations are frequent enough for 20 batches to see them
    feed = OnDeviceAugmentAMOS(store, ROI, rng=np.random.RandomState(11), flip_prob=0.5, rot_prob=0.5)
    res = {"device": torch.cuda.get_device_name(0), "host_threads": torch.get_num_threads(),
           "extents": [list(v[0].shape) for v in volumes], "flip_prob": 0.5, "rot_prob": 0.5, "shift_prob": 0.5, "batches": []}
    for batch in (4, 16):
        r = time_batch(volumes, feed, batch, dev)
        print(json.dumps(r), flush=True)
        res["batches"].append(r)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)
    if not all(r["equal"] for r in res["batches"]):
        raise SystemExit("device and host results differ")


if __name__ == "__main__":
    main()
