"""Simulated low resolution of the 3-D feed's intensity stage on the MI355X -> profiles/lowres_feed.json and profiles/lowres_feed.md.

usage (GPU box, from the repository root):
    python tools/lowres_feed_time.py [--parent PATH/libicl_hip.so] [--out profiles/lowres_feed]

The method is tools/intensity_feed_time.py's: one batch of 8 x 96^3 fp32 (28 MB); the stage leaves its result in the batch it was given,
so every variant runs on ROTATING batches (SETS buffers, together more than the 256 MiB Infinity Cache; every round starts from the
master batch again); the variants are timed INTERLEAVED in one process (round r: A, B, C, ..., A, B, ...), each window = LAUNCHES
back-to-back calls between two device events, the figure = window / LAUNCHES, and median, minimum and maximum over ROUNDS are recorded
after a warm-up of every variant.  Repeated application within a round changes the values (a low-resolution sample loses further
detail), not the work.

  stages      icl_intensity_lowres alone with every sample on, at zoom 0.5 (low extents 48^3) and zoom 0.9 (86^3): the gather and the
              copy back, two launches; and the whole five-transform chain through IntensityAugment.apply (noise, blur sigma 1, low
              resolution at zoom 0.5, statistics, contrast and gamma).  `copy` is Tensor.copy_ of the master batch into a rotating one
              (read 28 MB, write 28 MB): the yardstick.  A low-resolution stage that worked in place would have to move the same 2 x 28
              MB; this one writes the scratch buffer and copies it back, so it moves 4 (the gather's reads hit few distinct lines).
  context     the same transform on the host: the batch copied to the host, torch's interpolate twice per sample on the CPU, copied back.
  regression  only with --parent: (a) icl_volume_feed of this build against the parent commit's build, by tools/affine_feed_time.py's
              `measure`; (b) the four-transform chain of IntensityAugment.apply with rows of 11 (lowres_prob = 0: noise, blur,
              statistics, point, the launches of the parent) on this build, on this build again (the spread of the box) and on the
              parent's build, with the outputs compared bit for bit.  For (b) the binding's library handle is swapped for the
              duration of a call; the Python on top is this commit's in all three.

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
from icl_amd.dataloaders.intensity import IntensityAugment, lowres_extents  # noqa: E402
from icl_amd.utils.hashfill import hash_uniform_np  # noqa: E402

ROI = (96, 96, 96)
BATCH = 8
SETS = 12            # 12 x 28 MB = 340 MB
LAUNCHES = 50
ROUNDS = 11


def four_rows():
    """intensity_feed_time.py's rows: every one of the four older transforms on."""
    return [(1, 1000 + b, 0.1, 2.0, 1, 1.0, 1, 1.2 if b % 2 else 0.8, 1, 0.8 + 0.1 * b, b % 2) for b in range(BATCH)]


def five_rows(zoom=0.5):
    return [r + (1, zoom, zoom, zoom) for r in four_rows()]


def load_parent_chain(path):
    """The parent's build with the four entry points the older chain calls (it has no icl_intensity_lowres, so _lib cannot load it)."""
    lib = ctypes.CDLL(path)
    for name in ("icl_intensity_noise", "icl_intensity_blur", "icl_intensity_stats", "icl_intensity_point"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib._SIGNATURES[name]
    lib.icl_last_error.restype = ctypes.c_char_p
    return lib


def measure(dev, parent):
    L = _lib.lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    per = ROI[0] * ROI[1] * ROI[2]
    host = hash_uniform_np(BATCH * per, 9, 1.0).reshape(BATCH, 1, *ROI)
    master = torch.as_tensor(host).to(dev)
    pool = [master.clone() for _ in range(SETS)]
    scratch = torch.empty(16 * per, dtype=torch.float32, device=dev)
    turn = {"n": 0}

    def batch():
        turn["n"] = (turn["n"] + 1) % SETS
        return pool[turn["n"]]

    def lowres_params(zoom):
        low = lowres_extents(ROI, (zoom,) * 3)
        return (ctypes.c_int32 * (4 * BATCH))(*[v for _ in range(BATCH) for v in (1, *low)]), low

    p05, low05 = lowres_params(0.5)
    p09, low09 = lowres_params(0.9)
    stage = IntensityAugment(ROI)
    rows4, rows5 = four_rows(), five_rows()

    def call(name, *args):
        _lib.check(getattr(L, name)(*args), name)

    def chain4(lib):
        saved = _lib._lib
        _lib._lib = lib                                       # the binding's handle, for the duration of this call
        try:
            stage.apply(batch(), rows4)
        finally:
            _lib._lib = saved

    variants = {
        "copy": lambda: batch().copy_(master),
        "lowres_zoom0.5": lambda: call("icl_intensity_lowres", batch().data_ptr(), scratch.data_ptr(), p05, BATCH, *ROI, stream),
        "lowres_zoom0.9": lambda: call("icl_intensity_lowres", batch().data_ptr(), scratch.data_ptr(), p09, BATCH, *ROI, stream),
        "chain_five_transforms": lambda: stage.apply(batch(), rows5),
        "chain_four_transforms": lambda: chain4(L),
        "chain_four_transforms_again": lambda: chain4(L),
    }
    if parent is not None:
        variants["chain_four_transforms_parent"] = lambda: chain4(parent)

    def reset():
        for t in pool:
            t.copy_(master)

    # the four-transform chain once from the master batch on either build, for the bit comparison
    equal = None
    if parent is not None:
        results = []
        for lib in (L, parent):
            reset()
            turn["n"] = SETS - 1
            chain4(lib)
            torch.cuda.synchronize()
            results.append(pool[0].clone())
        equal = bool(torch.equal(results[0].view(torch.int32), results[1].view(torch.int32)))

    for fn in variants.values():
        aft.window(fn, SETS)
    times = {k: [] for k in variants}
    finite = True
    for _ in range(ROUNDS):
        reset()                                               # every round starts from the master batch
        for k, fn in variants.items():
            times[k].append(aft.window(fn, LAUNCHES))
        finite = finite and bool(all(torch.isfinite(t).all() for t in pool))
    med = {k: statistics.median(v) for k, v in times.items()}
    nbytes = 4 * BATCH * per
    copy_rate = 2 * nbytes / med["copy"]                      # bytes per microsecond
    moved = {"copy": 2, "lowres_zoom0.5": 2, "lowres_zoom0.9": 2}          # batches an in-place stage must read or write, at the least
    out = {"roi": list(ROI), "batch": BATCH, "batch_bytes": nbytes, "sets": SETS, "launches_per_window": LAUNCHES, "rounds": ROUNDS,
           "low_extents": {"zoom0.5": list(low05), "zoom0.9": list(low09)},
           "us_per_call": {k: {"median": round(med[k], 2), "min": round(min(v), 2), "max": round(max(v), 2)} for k, v in times.items()},
           "batches_moved_at_least": moved, "copy_gb_per_s": round(copy_rate / 1e3, 1),
           "fraction_of_copy_rate": {k: round(moved[k] * nbytes / med[k] / copy_rate, 3) for k in moved},
           "chain_four_spread_again_over_first": round(med["chain_four_transforms_again"] / med["chain_four_transforms"], 4),
           "finite_after_every_round": finite}
    if parent is not None:
        out["chain_four_now_over_parent"] = round(med["chain_four_transforms"] / med["chain_four_transforms_parent"], 4)
        out["chain_four_equal_to_parent"] = equal
    return out, host


def host_context(host, low):
    """The same transform with torch on the host for ONE batch already on the device: copy down, interpolate twice a sample, copy up."""
    import torch.nn.functional as F
    dev_batch = torch.as_tensor(host).cuda()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    x = dev_batch.cpu()
    t1 = time.perf_counter()
    for b in range(x.shape[0]):
        down = F.interpolate(x[b:b + 1], size=tuple(low), mode="nearest-exact")
        x[b:b + 1] = F.interpolate(down, size=ROI, mode="trilinear", align_corners=False)
    t2 = time.perf_counter()
    dev_batch.copy_(x)
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    return {"low_extents": list(low), "cpu_threads": torch.get_num_threads(), "copy_down_ms": round(1e3 * (t1 - t0), 1),
            "interpolate_ms": round(1e3 * (t2 - t1), 1), "copy_up_ms": round(1e3 * (t3 - t2), 1), "total_ms": round(1e3 * (t3 - t0), 1)}


def markdown(res):
    m = res["stages"]
    t = m["us_per_call"]
    lines = ["# Simulated low resolution in the intensity stage of the 3-D feed (`intensity_lowres_kernel`)", "",
             f"Written by `tools/lowres_feed_time.py` on one {res['device']}; the raw figures are in `lowres_feed.json`, the method in the tool's",
             f"docstring: one batch of {m['batch']} × 96³ ({m['batch_bytes'] / 1e6:.1f} MB) on {m['sets']} rotating batches, variants interleaved in one "
             f"process, {m['rounds']} rounds of {m['launches_per_window']} back-to-back calls between two device events after a warm-up.",
             "", "## 1. The stage", "",
             f"`copy` is `Tensor.copy_` of one batch ({m['copy_gb_per_s']} GB/s read + written).  The fraction is what an in-place stage would have to",
             "move (2 batches) over the time; the stage as built moves 4 (gather into the scratch buffer, copy back).", "",
             "| per call | median µs | min | max | fraction of the copy rate |", "|---|---|---|---|---|"]
    for k, v in t.items():
        lines.append(f"| `{k}` | {v['median']} | {v['min']} | {v['max']} | {m['fraction_of_copy_rate'].get(k, '')} |")
    c = res["host_one_batch"]
    lines += ["", "## 2. Context: the same transform on the host", "",
              f"One batch that is already on the device, copied to the host ({c['copy_down_ms']} ms), `interpolate` down to {tuple(c['low_extents'])} and "
              f"back up per sample on {c['cpu_threads']} CPU threads ({c['interpolate_ms']} ms), copied back ({c['copy_up_ms']} ms): "
              f"{c['total_ms']} ms, against {t['lowres_zoom0.5']['median'] / 1e3:.3f} ms for `lowres_zoom0.5` above.", "",
              "## 3. Regression check against the parent commit's build", ""]
    if "feed_96" in res:
        for key, name in (("feed_96", "96 × 96 × 96 (`volume_feed_kernel<4, false>`)"), ("feed_90", "96 × 96 × 90 (`volume_feed_kernel<1, false>`)")):
            b = res[key]
            u = b["us_per_call"]
            lines += [f"* `icl_volume_feed`, {name}: `plain` {u['plain']['median']} µs, `plain_again` {u['plain_again']['median']} µs (the same call twice a "
                      f"round: spread {b['spread_plain_again_over_plain']}), `plain_parent` {u['plain_parent']['median']} µs: **now / parent "
                      f"{b['now_over_parent']}**, outputs bit-equal: {b['equal'].get('plain_parent')}."]
        lines += [f"* the four-transform chain of `IntensityAugment.apply` (rows of 11): {t['chain_four_transforms']['median']} µs, again "
                  f"{t['chain_four_transforms_again']['median']} µs (spread {m['chain_four_spread_again_over_first']}), on the parent's build "
                  f"{t['chain_four_transforms_parent']['median']} µs: **now / parent {m['chain_four_now_over_parent']}**, outputs bit-equal: "
                  f"{m['chain_four_equal_to_parent']}."]
    else:
        lines += ["No parent library was given (`--parent`): NOT measured in this run."]
    lines.append("")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="libicl_hip.so of the parent commit's build, for the regression check")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lowres_feed"), help="path without extension: .json and .md are written")
    ap.add_argument("--notes", default=os.path.join(ROOT, "profiles", "lowres_feed_notes.md"),
                    help="a markdown file whose text is appended to the .md when it exists (what bounds the gather, open work)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lowres_feed_time.py needs a HIP device")
    dev = torch.device("cuda", 0)
    parent_chain = load_parent_chain(a.parent) if a.parent else None
    stages, host = measure(dev, parent_chain)
    res = {"device": torch.cuda.get_device_name(0), "stages": stages, "host_one_batch": host_context(host, stages["low_extents"]["zoom0.5"])}
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
