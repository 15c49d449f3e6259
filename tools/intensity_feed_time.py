"""The intensity stage of the 3-D feed on the MI355X -> profiles/intensity_feed.json and profiles/intensity_feed.md.

usage (GPU box, from the repository root):
    python tools/intensity_feed_time.py [--parent PATH/libicl_hip.so] [--out profiles/intensity_feed]

One batch of 8 x 96^3 fp32 (28 MB).  The stage works IN PLACE, so every variant runs on ROTATING batches (SETS buffers a pool, together more
than the 256 MiB Infinity Cache: a call never finds the lines its predecessor left in cache; one pool for noise, blur and the chain, one for
the pointwise variants, which run on the statistics of the master batch and keep every value inside its range; every round starts from
the master batch again); the variants are timed INTERLEAVED in one process
(round r: A, B, C, ..., A, B, ...), each window = LAUNCHES back-to-back calls between two device events, the figure = window / LAUNCHES,
and median, minimum and maximum over ROUNDS are recorded after a warm-up of every variant.  Repeated application within a round changes the values (noise accumulates, blur smooths further, about four applications a buffer), not the work.

  stages      each entry point alone with every sample on (noise sigma 0.1 clip 2; blur sigma 1.0, r = 4, and sigma 3.0, r = 12; the
              statistics; contrast alone; gamma alone; contrast + gamma), and the whole chain through IntensityAugment.apply, each as a
              fraction of the device copy rate for the bytes it must move: `copy` is Tensor.copy_ of the master batch into a rotating one (read 28 MB, write 28 MB);
              a pointwise stage must move the same 2 x 28 MB, the statistics read 28 MB, a blur reads and writes three times.
  context     the same chain on the host: the batch copied to the host, scipy's gaussian_filter and numpy for the rest (one core), and
              copied back.
  regression  icl_volume_feed of this build against the parent commit's build (only with --parent), interleaved on one box, by
              tools/affine_feed_time.py's method and code (its `measure`): those kernels do not change, so the ratio should sit inside the
              spread of the box.

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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import affine_feed_time as aft  # noqa: E402
from icl_amd import _lib  # noqa: E402
from icl_amd.dataloaders.amos import amos_volume_store  # noqa: E402
from icl_amd.dataloaders.intensity import INTENSITY_WS_DOUBLES, IntensityAugment, blur_weights  # noqa: E402
from icl_amd.utils.hashfill import hash_uniform_np  # noqa: E402

ROI = (96, 96, 96)
BATCH = 8
SETS = 12            # 12 x 28 MB = 340 MB
LAUNCHES = 50
ROUNDS = 11


def stage_rows():
    return [(1, 1000 + b, 0.1, 2.0, 1, 1.0, 1, 1.2 if b % 2 else 0.8, 1, 0.8 + 0.1 * b, b % 2) for b in range(BATCH)]


def measure(dev):
    L = _lib.lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    per = ROI[0] * ROI[1] * ROI[2]
    host = hash_uniform_np(BATCH * per, 9, 1.0).reshape(BATCH, 1, *ROI)
    master = torch.as_tensor(host).to(dev)
    # two pools: `free` for the variants whose values may wander (noise, blur, the chain, which takes its own statistics), `ranged` for
    # the pointwise variants, which run on the statistics of the master batch and keep every value inside its [min, max]
    free = [master.clone() for _ in range(SETS)]
    ranged = [master.clone() for _ in range(SETS)]
    scratch = torch.empty(16 * per, dtype=torch.float32, device=dev)
    stats = torch.zeros((BATCH, 4), dtype=torch.float32, device=dev)
    stats_out = torch.zeros((BATCH, 4), dtype=torch.float32, device=dev)
    ws = torch.empty(INTENSITY_WS_DOUBLES, dtype=torch.float64, device=dev)
    turn = {"n": 0}

    def batch(pool=free):
        turn["n"] = (turn["n"] + 1) % SETS
        return pool[turn["n"]]

    D = lambda vals: (ctypes.c_double * len(vals))(*vals)      # noqa: E731
    rows = stage_rows()
    noise_p = D([float(v) for r in rows for v in r[0:4]])

    def blur_p(sigma):
        w = list(blur_weights(sigma))
        return D([v for _ in rows for v in (1.0, sigma, *w, *([0.0] * (13 - len(w))))])

    blur1, blur3 = blur_p(1.0), blur_p(3.0)
    flags = (ctypes.c_int32 * BATCH)(*([1] * BATCH))
    point = lambda c, g: D([float(v) for r in rows for v in (c, r[7], g, r[9], r[10] if g else 0)])      # noqa: E731
    p_contrast, p_gamma, p_both = point(1, 0), point(0, 1), point(1, 1)
    stage = IntensityAugment(ROI)

    def call(name, *args):
        _lib.check(getattr(L, name)(*args), name)

    call("icl_intensity_stats", master.data_ptr(), flags, BATCH, *ROI, stats.data_ptr(), ws.data_ptr(), stream)
    variants = {
        "copy": lambda: batch().copy_(master),
        "noise": lambda: call("icl_intensity_noise", batch().data_ptr(), noise_p, BATCH, *ROI, stream),
        "blur_sigma1_r4": lambda: call("icl_intensity_blur", batch().data_ptr(), scratch.data_ptr(), blur1, BATCH, *ROI, stream),
        "blur_sigma3_r12": lambda: call("icl_intensity_blur", batch().data_ptr(), scratch.data_ptr(), blur3, BATCH, *ROI, stream),
        "stats": lambda: call("icl_intensity_stats", batch(ranged).data_ptr(), flags, BATCH, *ROI, stats_out.data_ptr(), ws.data_ptr(), stream),
        "contrast": lambda: call("icl_intensity_point", batch(ranged).data_ptr(), stats.data_ptr(), p_contrast, BATCH, *ROI, stream),
        "gamma": lambda: call("icl_intensity_point", batch(ranged).data_ptr(), stats.data_ptr(), p_gamma, BATCH, *ROI, stream),
        "contrast_gamma": lambda: call("icl_intensity_point", batch(ranged).data_ptr(), stats.data_ptr(), p_both, BATCH, *ROI, stream),
        "chain": lambda: stage.apply(batch(), rows),
    }

    def reset():
        for t in free + ranged:
            t.copy_(master)

    for fn in variants.values():
        aft.window(fn, SETS)
    times = {k: [] for k in variants}
    finite = True
    for _ in range(ROUNDS):
        reset()                                               # every round starts from the master batch
        for k, fn in variants.items():
            times[k].append(aft.window(fn, LAUNCHES))
        finite = finite and bool(all(torch.isfinite(t).all() for t in free + ranged))
    med = {k: statistics.median(v) for k, v in times.items()}
    nbytes = 4 * BATCH * per
    moved = {"copy": 2, "noise": 2, "blur_sigma1_r4": 6, "blur_sigma3_r12": 6, "stats": 1, "contrast": 2, "gamma": 2, "contrast_gamma": 2,
             "chain": 2 + 6 + 1 + 2}                           # batches read or written, at the least
    copy_rate = 2 * nbytes / med["copy"]                      # bytes per microsecond
    out = {"roi": list(ROI), "batch": BATCH, "batch_bytes": nbytes, "sets": SETS, "launches_per_window": LAUNCHES, "rounds": ROUNDS,
           "us_per_call": {k: {"median": round(med[k], 2), "min": round(min(v), 2), "max": round(max(v), 2)} for k, v in times.items()},
           "batches_moved": moved, "copy_gb_per_s": round(copy_rate / 1e3, 1),
           "fraction_of_copy_rate": {k: round(moved[k] * nbytes / med[k] / copy_rate, 3) for k in variants},
           "finite_after_every_round": finite}
    return out, host, rows


def host_context(host, rows):
    """The same chain with scipy / numpy on the host for ONE batch already on the device: copy down, transform, copy up (seconds)."""
    from scipy import ndimage
    dev_batch = torch.as_tensor(host).cuda()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    x = dev_batch.cpu().numpy()
    t1 = time.perf_counter()
    for b, r in enumerate(rows):
        v = x[b, 0]
        n = np.random.RandomState(r[1]).normal(0.0, r[2], v.shape).astype(np.float32)
        v = v + np.clip(n, -r[3] * r[2], r[3] * r[2])
        v = ndimage.gaussian_filter(v, r[5], mode="reflect", truncate=4.0)
        mn, mx, mean = v.min(), v.max(), v.mean()
        v = np.clip((v - mean) * np.float32(r[7]) + mean, mn, mx)
        mn, mx = v.min(), v.max()
        s = -1.0 if r[10] else 1.0
        lo = -mx if r[10] else mn
        v = (s * (np.power((s * v - lo) / (mx - mn + 1e-7), r[9]) * (mx - mn) + lo)).astype(np.float32)
        x[b, 0] = v
    t2 = time.perf_counter()
    dev_batch.copy_(torch.as_tensor(x))
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    return {"copy_down_ms": round(1e3 * (t1 - t0), 1), "transforms_ms": round(1e3 * (t2 - t1), 1), "copy_up_ms": round(1e3 * (t3 - t2), 1),
            "total_ms": round(1e3 * (t3 - t0), 1)}


def markdown(res):
    m = res["stages"]
    lines = ["# The intensity stage of the 3-D feed (`csrc/kernels/intensity.h`)", "",
             f"Written by `tools/intensity_feed_time.py` on one {res['device']}; the raw figures are in `intensity_feed.json`, the method in the",
             f"tool's docstring: one batch of {m['batch']} × 96³ ({m['batch_bytes'] / 1e6:.1f} MB), in place on {m['sets']} rotating batches, variants "
             f"interleaved in one process, {m['rounds']} rounds of {m['launches_per_window']} back-to-back calls between two device events after a warm-up.",
             "", "## 1. The stages", "",
             "`batches moved` is the least a stage must read or write, in batches; the last column is that many bytes over the time, as a fraction of",
             f"what `Tensor.copy_` of one batch reaches ({m['copy_gb_per_s']} GB/s read + written).", "",
             "| per call | median µs | min | max | batches moved | fraction of the copy rate |", "|---|---|---|---|---|---|"]
    for k, t in m["us_per_call"].items():
        lines.append(f"| `{k}` | {t['median']} | {t['min']} | {t['max']} | {m['batches_moved'][k]} | {m['fraction_of_copy_rate'][k]} |")
    c = res["host_chain_one_batch"]
    lines += ["", "## 2. Context: the same chain on the host", "",
              f"One batch that is already on the device, copied to the host ({c['copy_down_ms']} ms), transformed with scipy's `gaussian_filter` and numpy "
              f"on one core ({c['transforms_ms']} ms) and copied back ({c['copy_up_ms']} ms): {c['total_ms']} ms, against "
              f"{m['us_per_call']['chain']['median'] / 1e3:.3f} ms for `chain` above.", "",
              "## 3. Regression check: `icl_volume_feed` against the parent commit's build", ""]
    if "feed_96" in res:
        for key, name in (("feed_96", "96 × 96 × 96 (`volume_feed_kernel<4, false>`)"), ("feed_90", "96 × 96 × 90 (`volume_feed_kernel<1, false>`)")):
            b = res[key]
            t = b["us_per_call"]
            lines += [f"* {name}: `plain` {t['plain']['median']} µs, `plain_again` {t['plain_again']['median']} µs (the same call twice a round: spread "
                      f"{b['spread_plain_again_over_plain']}), `plain_parent` {t['plain_parent']['median']} µs: **now / parent {b['now_over_parent']}**, "
                      f"outputs bit-equal: {b['equal'].get('plain_parent')}."]
    else:
        lines += ["No parent library was given (`--parent`): NOT measured in this run."]
    lines.append("")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="libicl_hip.so of the parent commit's build, for the regression check")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "intensity_feed"), help="path without extension: .json and .md are written")
    ap.add_argument("--notes", default=os.path.join(ROOT, "profiles", "intensity_feed_notes.md"),
                    help="a markdown file whose text is appended to the .md when it exists (what bounds the blur, open work)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("intensity_feed_time.py needs a HIP device")
    dev = torch.device("cuda", 0)
    stages, host, rows = measure(dev)
    res = {"device": torch.cuda.get_device_name(0), "stages": stages, "host_chain_one_batch": host_context(host, rows)}
    if a.parent:
        parent = aft.load_parent(a.parent)
        store = amos_volume_store([aft.make_volume(j, s) for j, s in enumerate(aft.SHAPES)], dev)
        res["feed_96"], _, _ = aft.measure(_lib.lib(), parent, store, dev, (96, 96, 96), False)
        res["feed_90"], _, _ = aft.measure(_lib.lib(), parent, store, dev, (96, 96, 90), False)
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


if __name__ == "__main__":
    main()
