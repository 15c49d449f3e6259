"""Host (numpy / scipy) against device (kernels/metrics.h) validation metrics on the MI355X -> profiles/val_metric_time.json.

usage (GPU box, from the repository root):  python tools/val_metric_time.py [--reps 10] [--out profiles/val_metric_time.json]

Per shape (seeded synthetic ellipsoids with speckle noise, icl_amd.utils.hashfill.synthetic_segmentation; the last row also
scatters 2 % of the prediction's voxels over the whole volume):
  host_s       one call of [cal_metric(gt == c, pred == c) for every class] (host clock)
  upload_ms    host -> device copy of both label maps, synchronised (host clock; median of --reps)
  metric_ms    ops.seg_metrics + the copy of the records back, host clock around a synchronised call (median of --reps, after a warm-up)
  kernel_ms    device events around ops.seg_metrics alone (median)
  equal        the device result == the host result (values and types)
and one whole test_all_case_base on two 140x170x140 cases with a hash-filled unet_3D under ICL_VAL_METRICS=host and =device.
Kernel-by-kernel times: run it under `rocprofv3 --kernel-trace --stats` in a separate call.
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

from icl_amd import ops  # noqa: E402
from icl_amd.utils.hashfill import fill_like_reference_init, synthetic_segmentation, synthetic_volume  # noqa: E402
from icl_amd.val_3D import cal_metric, cal_metric_multiclass  # noqa: E402

# (name, shape, num_classes, seed, scatter)
SHAPES = [("brats_like_140x170x140_1class", (140, 170, 140), 2, 100, 0.0),
          ("240x240x155_1class", (240, 240, 155), 2, 101, 0.0),
          ("amos_like_256x256x128_15class", (256, 256, 128), 16, 102, 0.0),
          # the same organs, and 2 % of the prediction's voxels with a random class over the whole volume (every class's border spans it)
          ("amos_like_256x256x128_15class_scattered", (256, 256, 128), 16, 102, 0.02)]


def _sync():
    torch.cuda.synchronize()


def time_shape(name, shape, nc, reps, dev, seed, scatter=0.0):
    gt, pred = synthetic_segmentation(shape, nc, seed, speckle=0.02 if nc == 2 else 0.01, scatter=scatter)
    t0 = time.perf_counter()
    want = [cal_metric(gt == c, pred == c) for c in range(1, nc)]
    host_s = time.perf_counter() - t0
    up = []
    for _ in range(reps + 1):
        _sync()
        t0 = time.perf_counter()
        g, p = torch.from_numpy(gt).to(dev, non_blocking=False), torch.from_numpy(pred).to(dev, non_blocking=False)
        _sync()
        up.append((time.perf_counter() - t0) * 1e3)
    got = cal_metric_multiclass(g, p, nc)          # warm-up (code objects, allocator)
    metric, kern = [], []
    for _ in range(reps):
        _sync()
        t0 = time.perf_counter()
        got = cal_metric_multiclass(g, p, nc)
        metric.append((time.perf_counter() - t0) * 1e3)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.seg_metrics(p, g, nc)
        e1.record()
        _sync()
        kern.append(e0.elapsed_time(e1))
    equal = got == want and [[type(v) for v in m] for m in got] == [[type(v) for v in m] for m in want]
    return {"name": name, "shape": list(shape), "classes": nc - 1, "voxels": int(np.prod(shape)), "scatter": scatter, "host_s": round(host_s, 3),
            "upload_ms": round(statistics.median(up[1:]), 3), "metric_ms": round(statistics.median(metric), 3),
            "metric_ms_min": round(min(metric), 3), "kernel_ms": round(statistics.median(kern), 3), "equal": bool(equal)}


def time_test_all_case(dev):
    from icl_amd.networks.unet_3D import unet_3D
    from icl_amd.val_3D import test_all_case_base
    model = unet_3D(n_classes=2, in_channels=1, device=dev)
    fill_like_reference_init(list(model.named_parameters()))
    model.eval()
    cases = []
    for s in (0, 1):
        gt, _ = synthetic_segmentation((140, 170, 140), 2, 50 + s)
        cases.append((synthetic_volume((140, 170, 140), 60 + s).numpy() + gt.astype(np.float32), gt))
    out = {}
    for mode in ("device", "host", "device", "host"):      # the first pass of each warms up; the second is reported
        os.environ["ICL_VAL_METRICS"] = mode
        _sync()
        t0 = time.perf_counter()
        res = test_all_case_base(model, "unet_3D", None, num_classes=2, patch_size=(96, 96, 96), stride_xy=64, stride_z=64, cases=cases)
        _sync()
        out[mode] = {"s": round(time.perf_counter() - t0, 3), "metric_cal": res}
    os.environ.pop("ICL_VAL_METRICS", None)
    return {"cases": 2, "shape": [140, 170, 140], "patch": [96, 96, 96], "stride_xy": 64, "stride_z": 64,
            "device_s": out["device"]["s"], "host_s": out["host"]["s"], "equal": out["device"]["metric_cal"] == out["host"]["metric_cal"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "val_metric_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("val_metric_time.py needs a HIP device")
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "host_threads": torch.get_num_threads(), "shapes": []}
    for name, shape, nc, seed, scatter in SHAPES:
        r = time_shape(name, shape, nc, a.reps, dev, seed, scatter)
        print(json.dumps(r), flush=True)
        res["shapes"].append(r)
    res["test_all_case_base"] = time_test_all_case(dev)
    print(json.dumps(res["test_all_case_base"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)
    if not all(r["equal"] for r in res["shapes"]) or not res["test_all_case_base"]["equal"]:
        raise SystemExit("device and host metrics differ")


if __name__ == "__main__":
    main()
