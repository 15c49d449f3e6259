"""ATen loop against window kernels (kernels/window.h) in the 3-D sliding window of validation, on the MI355X -> profiles/val_window_time.json.

usage (GPU box, from the repository root):  python tools/val_window_time.py [--reps 10] [--out profiles/val_window_time.json]

Two bookkeeping cases with a predictor that returns pre-filled logits (no network: what is timed is the gather of the windows, the
soft-max / accumulation and the final division, arg-max and crop):
  brats_like   140 x 170 x 140, 2 classes, 96^3 windows, stride 64, four per forward   val_3D._single_case_on_device (soft-max form)
  amos_like    256 x 256 x 128, 16 classes, 96^3 windows, overlap 0.25, four per forward   val_3D.sliding_window_inference (logits form)
and one whole test_all_case_base on two 140 x 170 x 140 cases with a hash-filled unet_3D.  Per case, after one warm-up of each path,
--reps PAIRS are timed in one process, ICL_VAL_WINDOWS=device and =aten alternately (aten is the loop as it was before the kernels):
  event_ms     device events around the call (median, min, max over the pairs)
  host_ms      host clock around the call, ending in a device synchronise (median)
  diff_ms      device minus aten within each pair, event times: median, and min / max (the pair-to-pair spread)
  peak_bytes   torch.cuda.max_memory_allocated() above the allocation at the start of the call
  equal        every timed pair returned equal outputs (AMOS: the logits; BraTS bookkeeping: the label maps; test_all_case_base: the
               metric lists) — for the soft-max form, whose last bits may differ, label_mismatch and score_maxdiff are recorded too
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

from icl_amd import val_3D  # noqa: E402
from icl_amd.utils.hashfill import fill_like_reference_init, synthetic_segmentation, synthetic_volume  # noqa: E402


class Prefilled(torch.nn.Module):
    """Returns the first n of its pre-filled logits for a batch of n windows: the loops' bookkeeping alone."""

    def __init__(self, logits):
        super().__init__()
        self.anchor = torch.nn.Parameter(torch.zeros(1, device=logits.device), requires_grad=False)
        self.logits = logits

    def forward(self, x):
        return self.logits[:x.shape[0]]


def timed(fn):
    """(result, event ms, host ms, peak bytes above the start)."""
    torch.cuda.synchronize()
    start = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    host = (time.perf_counter() - t0) * 1e3
    return out, e0.elapsed_time(e1), host, torch.cuda.max_memory_allocated() - start


def alternate(fn, reps, compare):
    """One warm-up of each path, then `reps` pairs device / aten.  compare(device result, aten result) -> dict of bools / numbers."""
    rows = {"device": [], "aten": []}
    checks = []
    for rep in range(reps + 1):
        pair = {}
        for way in ("device", "aten"):
            os.environ["ICL_VAL_WINDOWS"] = way
            pair[way] = timed(fn)
        if rep == 0:
            continue
        for way in rows:
            rows[way].append(pair[way][1:])
        checks.append(compare(pair["device"][0], pair["aten"][0]))
        del pair
    os.environ.pop("ICL_VAL_WINDOWS", None)
    out = {}
    for way, r in rows.items():
        ev, host, peak = zip(*r)
        out[way] = {"event_ms": round(statistics.median(ev), 3), "event_ms_min": round(min(ev), 3), "event_ms_max": round(max(ev), 3),
                    "host_ms": round(statistics.median(host), 3), "peak_bytes": int(max(peak))}
    diffs = [d[0] - a[0] for d, a in zip(rows["device"], rows["aten"])]
    out["diff_ms"] = {"median": round(statistics.median(diffs), 3), "min": round(min(diffs), 3), "max": round(max(diffs), 3)}
    out["equal"] = all(c["equal"] for c in checks)
    for k in checks[0]:
        if k != "equal":
            out[k] = max(c[k] for c in checks)
    return out


def brats_like(dev, reps):
    shape, nc, patch = (140, 170, 140), 2, (96, 96, 96)
    net = Prefilled(synthetic_volume((4, nc) + patch, 7).to(dev))
    image = synthetic_volume(shape, 8).numpy()

    def compare(d, a):
        return {"equal": bool(torch.equal(d[0], a[0])), "label_mismatch": float((d[0] != a[0]).float().mean()),
                "score_maxdiff": float((d[1] - a[1]).abs().max())}
    r = alternate(lambda: val_3D._single_case_on_device(net, "unet_3D", image, 64, 64, patch, nc), reps, compare)
    r.update({"name": "brats_like_140x170x140_2class", "shape": list(shape), "classes": nc, "patch": list(patch), "stride": 64,
              "windows": int(np.prod([-(-(s - 96) // 64) + 1 for s in shape])),
              "form": "soft-max, label map + score (host -> device copy of the volume included)"})
    return r


def amos_like(dev, reps):
    shape, nc, roi = (256, 256, 128), 16, (96, 96, 96)
    logits = synthetic_volume((4, nc) + roi, 9).to(dev)
    x = synthetic_volume((1, 1) + shape, 10).to(dev)
    windows = int(np.prod([len(val_3D._scan_starts(s, 96, 0.25)) for s in shape]))
    r = alternate(lambda: val_3D.sliding_window_inference(x, roi, 4, lambda win: logits[:win.shape[0]]), reps,
                  lambda d, a: {"equal": bool(torch.equal(d, a))})
    r.update({"name": "amos_like_256x256x128_16class", "shape": list(shape), "classes": nc, "patch": list(roi), "overlap": 0.25,
              "windows": windows, "form": "logits, averaged logits returned"})
    return r


def whole_validation(dev, reps):
    from icl_amd.networks.unet_3D import unet_3D
    model = unet_3D(n_classes=2, in_channels=1, device=dev)
    fill_like_reference_init(list(model.named_parameters()))
    model.eval()
    cases = []
    for s in (0, 1):
        gt, _ = synthetic_segmentation((140, 170, 140), 2, 50 + s)
        cases.append((synthetic_volume((140, 170, 140), 60 + s).numpy() + gt.astype(np.float32), gt))
    r = alternate(lambda: val_3D.test_all_case_base(model, "unet_3D", None, num_classes=2, patch_size=(96, 96, 96), stride_xy=64, stride_z=64,
                                                    cases=cases), reps, lambda d, a: {"equal": d == a})
    r.update({"name": "test_all_case_base_2x140x170x140_unet_3D", "cases": 2, "shape": [140, 170, 140], "patch": [96, 96, 96], "stride": 64})
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "val_window_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("val_window_time.py needs a HIP device")
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "bookkeeping": []}
    for fn in (brats_like, amos_like):
        r = fn(dev, a.reps)
        print(json.dumps(r), flush=True)
        res["bookkeeping"].append(r)
    res["test_all_case_base"] = whole_validation(dev, a.reps)
    print(json.dumps(res["test_all_case_base"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)
    if not res["bookkeeping"][1]["equal"]:
        raise SystemExit("device and aten logits differ")


if __name__ == "__main__":
    main()
