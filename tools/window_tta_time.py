"""Mirror test-time augmentation in the sliding-window kernels (kernels/window.h) on the MI355X -> profiles/window_tta_time.json.

usage (GPU box, from the repository root):  python tools/window_tta_time.py [--reps 20] [--out profiles/window_tta_time.json]

launches   one launch of 16 passes of 96^3 over a 160^3 volume (origins on a 2 x 2 x 4 grid, all multiples of 4: the quad forms), C = 2
           (soft-max form, the BraTS loop) and C = 16 (logits form, the AMOS loop), constant weights:
             plain     ops.window_gather / window_accumulate without ``flips``  (window_gather_kernel<4>, window_accumulate_kernel<NC, 4>)
             mask0     ``flips=[0] * 16``   the WinFlips instantiations, nothing mirrored
             mask7     ``flips=[7] * 16``   every axis mirrored: reversed rows, reversed quads
           After a warm-up of every variant, --reps rounds; in a round the variants run one after the other (interleaved A/B/C), each as
           10 back-to-back launches between two device events.  us_per_launch: median, min, max over the rounds; gbytes_per_s: the bytes the
           launch has to move (gather: the windows read and written; accumulate: the logits read, score and weight maps of the bounding
           box read and written) over the median.
validation one ``test_single_case_base`` of a 160 x 160 x 96 volume (96^3 windows, stride 64: 4 windows, 4 passes per forward) on a
           hash-filled unet_3D with 2 classes, with ``mirror_axes=None`` (1 forward) and ``(0, 1, 2)`` (32 passes, 8 forwards), alternating,
           host clock around the call (it ends with the copy of the label map to the host).
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

import torch  # noqa: E402

from icl_amd import ops, val_3D  # noqa: E402
from icl_amd.utils.hashfill import fill_like_reference_init, synthetic_volume  # noqa: E402

INNER = 10
ROI, PSIZE = (96, 96, 96), (160, 160, 160)
ORIGINS = [(z, y, x) for z in (0, 64) for y in (0, 64) for x in (0, 16, 32, 64)]
VARIANTS = {"plain": None, "mask0": [0] * 16, "mask7": [7] * 16}


def stats(us):
    return {"median": round(statistics.median(us), 2), "min": round(min(us), 2), "max": round(max(us), 2)}


def events_us(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(INNER):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / INNER


def launches(dev, nc, softmax, reps):
    vol = synthetic_volume((1,) + PSIZE, 3).to(dev)
    win = torch.empty((16, 1) + ROI, device=dev)
    logits = synthetic_volume((16, nc) + ROI, 4).to(dev)
    score = torch.zeros((nc,) + PSIZE, device=dev)
    weight = torch.zeros(PSIZE, device=dev)
    calls = {}
    for name, flips in VARIANTS.items():
        calls["gather_" + name] = lambda f=flips: ops.window_gather(vol, ORIGINS, ROI, (0, 0, 0), PSIZE, out=win, flips=f)
        calls["accumulate_" + name] = lambda f=flips: ops.window_accumulate(logits, ORIGINS, score, weight, None, softmax=softmax, flips=f)
    rows = {k: [] for k in calls}
    for rep in range(reps + 1):
        for k, fn in calls.items():
            t = events_us(fn)
            if rep:
                rows[k].append(t)
    p = ROI[0] * ROI[1] * ROI[2]
    box = (64 + 96) * (64 + 96) * (64 + 96)
    nbytes = {"gather": 2 * 16 * p * 4, "accumulate": 16 * nc * p * 4 + 2 * (nc + 1) * box * 4}
    out = {"classes": nc, "form": "soft-max" if softmax else "logits", "passes_per_launch": 16, "launches_per_sample": INNER, "rounds": reps}
    for k, us in rows.items():
        s = stats(us)
        s["gbytes_per_s"] = round(nbytes[k.split("_")[0]] / (s["median"] * 1e-6) / 1e9, 1)
        out[k] = {"us_per_launch": s}
    for kind in ("gather", "accumulate"):
        for m in ("mask0", "mask7"):
            ratio = [a / b for a, b in zip(rows[f"{kind}_{m}"], rows[f"{kind}_plain"])]
            out[f"{kind}_{m}"]["over_plain"] = stats(ratio)
    return out


def validation(dev, reps):
    from icl_amd.networks.unet_3D import unet_3D
    model = unet_3D(n_classes=2, in_channels=1, device=dev)
    fill_like_reference_init(list(model.named_parameters()))
    model.eval()
    image = synthetic_volume((160, 160, 96), 21).numpy()
    rows = {"none": [], "all_mirrors": []}
    labels = {}
    for rep in range(reps + 1):
        for name, axes in (("none", None), ("all_mirrors", (0, 1, 2))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            labels[name] = val_3D.test_single_case_base(model, "unet_3D", image, 64, 64, ROI, num_classes=2, mirror_axes=axes)
            torch.cuda.synchronize()
            if rep:
                rows[name].append((time.perf_counter() - t0) * 1e3)
    out = {"volume": [160, 160, 96], "patch": list(ROI), "stride": 64, "windows": 4, "passes": {"none": 4, "all_mirrors": 32},
           "forwards": {"none": 1, "all_mirrors": 8}, "rounds": reps,
           "labels_that_differ": float((labels["none"] != labels["all_mirrors"]).mean())}
    for k, ms in rows.items():
        out[k] = {"host_ms": stats(ms)}
    out["all_mirrors_over_none"] = stats([a / b for a, b in zip(rows["all_mirrors"], rows["none"])])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--val-reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window_tta_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("window_tta_time.py needs a HIP device")
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "launches": []}
    for nc, softmax in ((2, True), (16, False)):
        r = launches(dev, nc, softmax, a.reps)
        print(json.dumps(r), flush=True)
        res["launches"].append(r)
    res["validation"] = validation(dev, a.val_reps)
    print(json.dumps(res["validation"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
