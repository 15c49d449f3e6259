"""Connected-component post-processing on the device (kernels/components.h) against the scipy host path on the same maps, on the MI355X
-> the "Times" section of profiles/val_components.md.

usage (GPU box, from the repository root):  python tools/val_components_time.py [--reps 10] [--out profiles/val_components.md]

Maps: seeded synthetic predictions (ellipsoids with speckle noise, 2 % of the voxels scattered over the volume) at 96^3 with 2 and 16
classes and at 160 x 160 x 48 with 4 classes; int64, as the arg-max yields them.  ``keep_components(map, num_classes)`` with its
defaults (largest component of each class, 6 neighbours).  Per map:
  host_ms     the scipy path on a host array (one scipy.ndimage.label per class; host clock, median of --reps)
  round_ms    the scipy path on the DEVICE tensor (ICL_VAL_COMPONENTS=host: copy down, scipy, copy up) — what a validation loop paid
              before; host clock around a synchronised call (median)
  device_ms   the kernels on the device tensor, host clock around a synchronised call (median, after a warm-up)
  kernel_ms   device events around ops.seg_filter_components alone (median)
  equal       the device result equals the host result voxel for voxel
No time is asserted: the figures are reported against the host path.  Kernel-by-kernel times: run it under a kernel trace in a
separate call.
"""
from __future__ import annotations

import argparse
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
from icl_amd.val_3D import keep_components  # noqa: E402

MAPS = [("96^3, 2 classes", (96, 96, 96), 2), ("96^3, 16 classes", (96, 96, 96), 16), ("160 x 160 x 48, 4 classes", (160, 160, 48), 4)]
BEGIN, END = "<!-- times: begin -->", "<!-- times: end -->"


def _median_ms(fn, reps, sync=None):
    out = []
    for _ in range(reps):
        if sync:
            sync()
        t0 = time.perf_counter()
        fn()
        if sync:
            sync()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def time_map(name, shape, nc, reps, dev, seed):
    _, pred = synthetic_segmentation(shape, nc, seed, scatter=0.02)
    pred = np.ascontiguousarray(pred.astype(np.int64))
    t = torch.from_numpy(pred).to(dev)
    sync = torch.cuda.synchronize
    host_ms = _median_ms(lambda: keep_components(pred, nc), max(3, reps // 3))
    want = keep_components(pred, nc)
    os.environ["ICL_VAL_COMPONENTS"] = "host"
    round_ms = _median_ms(lambda: keep_components(t, nc), max(3, reps // 3), sync)
    os.environ["ICL_VAL_COMPONENTS"] = "device"
    got = keep_components(t, nc)      # warm-up
    device_ms = _median_ms(lambda: keep_components(t, nc), reps, sync)
    kern = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ops.seg_filter_components(t, nc)
        b.record()
        sync()
        kern.append(a.elapsed_time(b))
    return {"name": name, "voxels": int(pred.size), "host_ms": host_ms, "round_ms": round_ms, "device_ms": device_ms,
            "kernel_ms": statistics.median(kern), "equal": bool(np.array_equal(got.cpu().numpy(), want))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "val_components.md"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    dev = torch.device("cuda", 0)
    rows = [time_map(name, shape, nc, args.reps, dev, 50 + i) for i, (name, shape, nc) in enumerate(MAPS)]
    lines = [f"Measured with `tools/val_components_time.py --reps {args.reps}` on {torch.cuda.get_device_name(0)}; medians, milliseconds.",
             "", "| map | voxels | host (scipy) | device tensor through scipy | device (kernels), synchronised | kernels alone | equal |",
             "|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['name']} | {r['voxels']:,} | {r['host_ms']:.2f} | {r['round_ms']:.2f} | {r['device_ms']:.3f} | {r['kernel_ms']:.3f} | "
                     f"{'yes' if r['equal'] else 'NO'} |")
        print(r)
    with open(args.out) as f:
        text = f.read()
    head, rest = text.split(BEGIN, 1)
    _, tail = rest.split(END, 1)
    with open(args.out, "w") as f:
        f.write(head + BEGIN + "\n" + "\n".join(lines) + "\n" + END + tail)
    return 0 if all(r["equal"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
