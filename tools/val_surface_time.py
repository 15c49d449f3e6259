"""Host (numpy / scipy) against device (kernels/metrics_surface.h) surface metrics with a voxel spacing on the MI355X
-> profiles/val_surface_time.json.

usage (GPU box, from the repository root):  python tools/val_surface_time.py [--reps 10] [--out profiles/val_surface_time.json]

The four cases of tools/val_metric_time.py (seeded synthetic ellipsoids with speckle noise; the last row also scatters 2 % of the
prediction's voxels over the whole volume), at spacing (1.5, 1.5, 2.0) and tolerance 1.0.  Per case:
  host_s          ONE call of the host restatement of all seven quantities for every class (surface_metrics_multiclass on numpy arrays; host clock)
  surface_ms      surface_metrics_multiclass on device tensors — ops.seg_surface_metrics + the copy of the records back — host clock around a
                  synchronised call (median of --reps, after a warm-up)
  kernel_ms       device events around ops.seg_surface_metrics alone (median)
  integer_ms      the integer path on the same maps, ops.seg_metrics + the copy back, host clock, synchronised (median): the baseline that is
                  not the code under test (voxel units, Dice and HD95 only)
  integer_kernel_ms  device events around ops.seg_metrics alone (median)
  agree           dice, hd95, hd, nsd of the device equal the host's bit for bit (dyadic spacing); the averages within (n + 4) 2^-52
The two device paths alternate inside one loop, so they see the same machine state.  No time is asserted.  Kernel-by-kernel times: run
it under `rocprofv3 --kernel-trace --stats` in a separate call.
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
from icl_amd.utils.hashfill import synthetic_segmentation  # noqa: E402
from icl_amd.val_3D import cal_metric_multiclass, surface_metrics_multiclass  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tools"))
from val_metric_time import SHAPES  # noqa: E402

SPACING = (1.5, 1.5, 2.0)
TOLERANCE = 1.0


def _sync():
    torch.cuda.synchronize()


def _agree(got, want, borders):
    for g, w, n in zip(got, want, borders):
        for k in ("dice", "hd95", "hd", "nsd"):
            if g[k] != w[k] or type(g[k]) is not type(w[k]):
                return False
        for k in ("assd", "asd_pred_gt", "asd_gt_pred"):
            if abs(g[k] - w[k]) > (n + 4) * 2.0 ** -52 * abs(w[k]):
                return False
    return True


def time_shape(name, shape, nc, reps, dev, seed, scatter=0.0):
    gt, pred = synthetic_segmentation(shape, nc, seed, speckle=0.02 if nc == 2 else 0.01, scatter=scatter)
    t0 = time.perf_counter()
    want = surface_metrics_multiclass(gt, pred, nc, SPACING, TOLERANCE)
    host_s = time.perf_counter() - t0
    g, p = torch.from_numpy(gt).to(dev), torch.from_numpy(pred).to(dev)
    got = surface_metrics_multiclass(g, p, nc, SPACING, TOLERANCE)      # warm-up (code objects, allocator)
    cal_metric_multiclass(g, p, nc)
    counts = ops.seg_surface_metrics(p, g, nc, SPACING, TOLERANCE)[0].cpu().tolist()
    surface, kern, integer, ikern = [], [], [], []
    for _ in range(reps):
        _sync()
        t0 = time.perf_counter()
        got = surface_metrics_multiclass(g, p, nc, SPACING, TOLERANCE)
        surface.append((time.perf_counter() - t0) * 1e3)
        _sync()
        t0 = time.perf_counter()
        cal_metric_multiclass(g, p, nc)
        integer.append((time.perf_counter() - t0) * 1e3)
        for fn, sink in ((lambda: ops.seg_surface_metrics(p, g, nc, SPACING, TOLERANCE), kern), (lambda: ops.seg_metrics(p, g, nc), ikern)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            _sync()
            sink.append(e0.elapsed_time(e1))
    med = lambda v: round(statistics.median(v), 3)  # noqa: E731
    return {"name": name, "shape": list(shape), "classes": nc - 1, "voxels": int(np.prod(shape)), "scatter": scatter,
            "spacing": list(SPACING), "tolerance": TOLERANCE, "host_s": round(host_s, 3), "surface_ms": med(surface),
            "surface_ms_min": round(min(surface), 3), "kernel_ms": med(kern), "integer_ms": med(integer), "integer_kernel_ms": med(ikern),
            "workspace_mib": round(ops._lib.lib().icl_seg_surface_ws_bytes(*shape, nc) / 2 ** 20, 1),
            "agree": bool(_agree(got, want, [max(c[3], c[4]) for c in counts]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "val_surface_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("val_surface_time.py needs a HIP device")
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "host_threads": torch.get_num_threads(), "reps": a.reps, "shapes": []}
    for name, shape, nc, seed, scatter in SHAPES:
        r = time_shape(name, shape, nc, a.reps, dev, seed, scatter)
        print(json.dumps(r), flush=True)
        res["shapes"].append(r)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)
    if not all(r["agree"] for r in res["shapes"]):
        raise SystemExit("device and host surface metrics differ")


if __name__ == "__main__":
    main()
