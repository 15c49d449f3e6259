"""Host (scipy / numpy) against device (slice_augment_kernel / slice_resize_kernel) 2-D data feed on the MI355X
-> profiles/feed2d_timing.json.

usage (GPU box, from the repository root):  python tools/feed2d_timing.py [--batches 60] [--out profiles/feed2d_timing.json]

Per configuration (hash-filled 256 x 216 slices; 24 -> 256 x 256, the U-Net trainer's batch, and 16 -> 224 x 224, the Swin-UNet one):
  scipy_ms     the reference's operations called directly from scipy / numpy in ONE process for the whole batch, with the draws of
               dataloaders/dataset.py:156-159: np.rot90 / np.flip(...).copy(), ndimage.rotate(order=0, reshape=False), two
               zoom(order=0), the torch.from_numpy casts and the collation (torch.stack); host clock, median of --batches
  device_ms    OnDeviceAugment2D.batch including its host-side draws, synchronised; host clock, median of --batches after a warm-up
  kernel_ms    device events around the same call (median)
  equal        every timed device batch == the scipy batch under the same seeds, bit for bit
and for a 10 x 256 x 216 case the two resizes of val_2D (in: slices -> 256 x 256 ready on the device as the network's input; back:
a device arg-max map -> 256 x 216 ready on the device for the metric kernels) with scipy on the host and with icl_slice_resize.
The baseline is scipy itself, not this package's host classes.  The reference runs its loader in eight worker processes; divide
scipy_ms by the workers you would give it.
"""
from __future__ import annotations

import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from scipy import ndimage  # noqa: E402
from scipy.ndimage import zoom  # noqa: E402

from icl_amd.dataloaders.dataset import DeviceSliceStore, OnDeviceAugment2D, resize_slices  # noqa: E402
from icl_amd.utils.hashfill import synthetic_labels, synthetic_volume  # noqa: E402

# (name, batch, slice extent, patch)
CONFIGS = [("unet_24x256x216_to_256x256", 24, (256, 216), (256, 256)), ("swinunet_16x256x216_to_224x224", 16, (256, 216), (224, 224))]
VAL_CASE = (10, 256, 216)
VAL_PATCH = (256, 256)
WARMUP = 5


def _sync():
    torch.cuda.synchronize()


def _seed(s):
    random.seed(s)
    np.random.seed(s)


def scipy_batch(slices, patch):
    """The reference's RandomGenerator per sample + the DataLoader's collation, from scipy / numpy directly."""
    images, labels = [], []
    for image, label in slices:
        if random.random() > 0.5:
            k = np.random.randint(0, 4)
            axis = np.random.randint(0, 2)
            image = np.flip(np.rot90(image, k), axis=axis).copy()
            label = np.flip(np.rot90(label, k), axis=axis).copy()
        elif random.random() > 0.5:
            angle = np.random.randint(-20, 20)
            image = ndimage.rotate(image, angle, order=0, reshape=False)
            label = ndimage.rotate(label, angle, order=0, reshape=False)
        x, y = image.shape
        image = zoom(image, (patch[0] / x, patch[1] / y), order=0)
        label = zoom(label, (patch[0] / x, patch[1] / y), order=0)
        images.append(torch.from_numpy(image.astype(np.float32)).unsqueeze(0))
        labels.append(torch.from_numpy(label.astype(np.uint8)))
    return torch.stack(images), torch.stack(labels)


def time_feed(name, batch, extent, patch, batches, dev):
    slices = [(synthetic_volume(extent, 7000 + i).numpy(), synthetic_labels(extent, 8000 + i, 4).numpy().astype(np.uint8))
              for i in range(batch)]
    store = DeviceSliceStore(slices, dev)
    feed = OnDeviceAugment2D(store, patch)
    idx = list(range(batch))
    host, device, kern, equal = [], [], [], True
    for n in range(WARMUP + batches):
        _seed(100 + n)
        t0 = time.perf_counter()
        want_image, want_label = scipy_batch(slices, patch)
        t_host = (time.perf_counter() - t0) * 1e3
        _seed(100 + n)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        _sync()
        t0 = time.perf_counter()
        e0.record()
        got = feed.batch(idx)
        e1.record()
        _sync()
        t_dev = (time.perf_counter() - t0) * 1e3
        if n >= WARMUP:
            host.append(t_host)
            device.append(t_dev)
            kern.append(e0.elapsed_time(e1))
            equal = equal and torch.equal(got["image"].cpu(), want_image) and torch.equal(got["label"].cpu(), want_label)
    return {"name": name, "batch": batch, "extent": list(extent), "patch": list(patch), "batches": batches,
            "scipy_ms": round(statistics.median(host), 3), "scipy_ms_min": round(min(host), 3),
            "device_ms": round(statistics.median(device), 3), "device_ms_min": round(min(device), 3),
            "kernel_ms": round(statistics.median(kern), 3), "equal": bool(equal)}


def time_val_resize(batches, dev):
    n, x, y = VAL_CASE
    image = synthetic_volume(VAL_CASE, 9000).numpy()
    maps = synthetic_labels((n,) + VAL_PATCH, 9001, 4).to(dev)                      # stands for the arg-max of the logits
    t = {"host_in": [], "host_back": [], "device_in": [], "device_back": []}
    equal = True
    for r in range(WARMUP + batches):
        _sync()
        t0 = time.perf_counter()
        resized = np.stack([zoom(image[i], (VAL_PATCH[0] / x, VAL_PATCH[1] / y), order=0) for i in range(n)])
        h_in = torch.from_numpy(resized).unsqueeze(1).float().to(dev)
        _sync()
        t1 = time.perf_counter()
        out = maps.cpu().numpy()
        pred = np.zeros((n, x, y), dtype=np.int64)
        for i in range(n):
            pred[i] = zoom(out[i], (x / VAL_PATCH[0], y / VAL_PATCH[1]), order=0)
        h_back = torch.from_numpy(pred).to(dev)
        _sync()
        t2 = time.perf_counter()
        d_in = resize_slices(torch.from_numpy(image).float().to(dev), VAL_PATCH).unsqueeze(1)
        _sync()
        t3 = time.perf_counter()
        d_back = resize_slices(maps, (x, y))
        _sync()
        t4 = time.perf_counter()
        if r >= WARMUP:
            for key, v in (("host_in", t1 - t0), ("host_back", t2 - t1), ("device_in", t3 - t2), ("device_back", t4 - t3)):
                t[key].append(v * 1e3)
            equal = equal and torch.equal(h_in, d_in) and torch.equal(h_back, d_back)
    res = {"case": list(VAL_CASE), "patch": list(VAL_PATCH), "repeats": batches, "equal": bool(equal)}
    for key, v in t.items():
        res[key + "_ms"] = round(statistics.median(v), 3)
    res["host_ms"] = round(res["host_in_ms"] + res["host_back_ms"], 3)
    res["device_ms"] = round(res["device_in_ms"] + res["device_back_ms"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=60)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feed2d_timing.json"))
    a = ap.parse_args()
    if a.batches < 50:
        raise SystemExit("feed2d_timing.py: at least 50 timed batches")
    if not torch.cuda.is_available():
        raise SystemExit("feed2d_timing.py needs a HIP device")
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "host_threads": torch.get_num_threads(), "feed": []}
    for name, batch, extent, patch in CONFIGS:
        r = time_feed(name, batch, extent, patch, a.batches, dev)
        print(json.dumps(r), flush=True)
        res["feed"].append(r)
    res["val_resize"] = time_val_resize(a.batches, dev)
    print(json.dumps(res["val_resize"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)
    if not all(r["equal"] for r in res["feed"]) or not res["val_resize"]["equal"]:
        raise SystemExit("device and scipy results differ")
    slower = [r["name"] for r in res["feed"] if r["device_ms"] >= r["scipy_ms"]]
    if res["val_resize"]["device_ms"] >= res["val_resize"]["host_ms"]:
        slower.append("val_resize")
    if slower:
        raise SystemExit("the device path is not below scipy for: " + ", ".join(slower))


if __name__ == "__main__":
    main()
