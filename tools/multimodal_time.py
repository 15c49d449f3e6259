"""Measurements of the multi-modal feed on the MI355X -> profiles/multimodal.md (written by hand from the JSON this tool prints).

usage (GPU box, from the repository root):
    python tools/multimodal_time.py feed  [--out FILE.json]     wall time of the two ways to form a 2 x 4 x 96^3 batch, from events
    python tools/multimodal_time.py feed --launches 20          the same calls, few of them: the run to put under
                                                                `rocprofv3 --kernel-trace --stats` for the kernel times
    python tools/multimodal_time.py conv  [--out FILE.json]     first convolution 4 -> 16 and 1 -> 16 at 2 x 96^3, forward + backward (for the trace)
    python tools/multimodal_time.py step  [--out FILE.json]     step time of the headline configuration at in_channels 4 and 1

feed:  2 samples x 4 channels x 96^3 from 240 x 240 x 155 sources.  `channels` is OnDeviceAugment.batch over a [4,W,H,D] store (one
       icl_crop_rotflip_channels launch); `stacked` is the only way the code before this feed could form the batch: four single-channel
       OnDeviceAugment.batch calls (icl_crop_rotflip) over per-modality stores with the same rows, and torch.stack on the channel axis;
       `copy` is Tensor.copy_ of the image batch (28.3 MB read + 28.3 MB written), the device copy rate of the day.  The three are timed
       INTERLEAVED in one process (round r: channels, stacked, copy, channels, ...), each window = LAUNCHES back-to-back calls between two
       device events after a warm-up, median / min / max over ROUNDS.  The outputs of the two ways are compared bit for bit.  Bytes the
       batch must move: image read + written (2 x 28.3 MB), label read (1.77 MB uint8) + written (14.2 MB int64).
No threshold is asserted: this tool records.
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

PATCH = (96, 96, 96)
SOURCE = (240, 240, 155)
CHANNELS = 4
VOLUMES = 4
ROUNDS = 11


def window(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches      # microseconds a call


def feed(dev, launches):
    from icl_amd.dataloaders.brats2019 import DeviceVolumeStore, OnDeviceAugment, draw_rotflip_crop
    g = torch.Generator(device="cpu").manual_seed(5)
    images = [torch.rand((CHANNELS, *SOURCE), generator=g) for _ in range(VOLUMES)]
    labels = [(torch.rand(SOURCE, generator=g) * 4).to(torch.uint8) for _ in range(VOLUMES)]
    multi = DeviceVolumeStore.from_device_tensors([i.to(dev) for i in images], [lab.to(dev) for lab in labels], dev)
    singles = [DeviceVolumeStore.from_device_tensors([m[c].contiguous() for m in multi.images], multi.labels, dev) for c in range(CHANNELS)]
    feed_multi = OnDeviceAugment(multi, PATCH)
    feed_single = [OnDeviceAugment(s, PATCH) for s in singles]
    np.random.seed(9)
    draws = [[draw_rotflip_crop(SOURCE, PATCH) for _ in range(2)] for _ in range(16)]      # 16 batches of rows, used in turn
    turn = {"n": 0}

    def rows():
        turn["n"] = (turn["n"] + 1) % len(draws)
        return [(turn["n"] + j) % VOLUMES for j in range(2)], draws[turn["n"]]

    def channels():
        idx, r = rows()
        return feed_multi.batch(idx, params=r)

    def stacked():
        idx, r = rows()
        outs = [f.batch(idx, params=r) for f in feed_single]
        return {"image": torch.stack([o["image"][:, 0] for o in outs], dim=1), "label": outs[0]["label"]}

    src = torch.rand((2, CHANNELS, *PATCH), device=dev)
    dst = torch.empty_like(src)
    variants = {"channels": channels, "stacked": stacked, "copy": lambda: dst.copy_(src)}
    turn["n"] = 0
    a = channels()
    turn["n"] = 0
    b = stacked()
    equal = bool(torch.equal(a["image"], b["image"]) and torch.equal(a["label"], b["label"]))
    for fn in variants.values():
        window(fn, 10)
    times = {k: [] for k in variants}
    for _ in range(ROUNDS if launches >= 50 else 1):
        for k, fn in variants.items():
            times[k].append(window(fn, launches))
    med = {k: statistics.median(v) for k, v in times.items()}
    vox = PATCH[0] * PATCH[1] * PATCH[2]
    image_bytes = 2 * CHANNELS * vox * 4
    moved = 2 * image_bytes + 2 * vox * (1 + 8)
    copy_rate = 2 * image_bytes / med["copy"]               # bytes per microsecond
    return {"patch": list(PATCH), "source": list(SOURCE), "batch": 2, "channels": CHANNELS, "launches_per_window": launches,
            "rounds": len(times["copy"]), "outputs_bit_equal": equal,
            "us_per_call": {k: {"median": round(med[k], 2), "min": round(min(v), 2), "max": round(max(v), 2)} for k, v in times.items()},
            "bytes_moved": moved, "copy_gb_per_s": round(copy_rate / 1e3, 1),
            "stacked_over_channels_wall": round(med["stacked"] / med["channels"], 3),
            "channels_fraction_of_copy_rate_wall": round(moved / med["channels"] / copy_rate, 3)}


def conv(dev, launches):
    """Forward and backward of the first convolution at 2 x 96^3, four input channels (the generic route) and one (conv_cin1.h), for a
    kernel trace; the wall time of forward + backward is returned for orientation only."""
    from icl_amd import ops
    out = {}
    for cin in (4, 1):
        x = torch.randn(2, cin, 96, 96, 96, device=dev)
        w = (torch.randn(16, cin, 3, 3, 3, device=dev) * 0.2).requires_grad_()
        b = torch.randn(16, device=dev) * 0.1
        g = torch.randn(2, 16, 96, 96, 96, device=dev)
        route = ops.plan_conv3d(x.shape, w.shape, x_needs_grad=False, has_bias=True, zero_bias_grad=True)

        def fn():
            w.grad = None
            ops.conv3d(x, w, b, zero_bias_grad=True).backward(g)
        window(fn, 3)
        out[f"cin{cin}"] = {"route": str(route), "fwd_bwd_us_wall": round(window(fn, launches), 1)}
    return out


def step(dev, steps):
    from icl_amd.networks.unet_3D_icl import unet_3D_icl
    from icl_amd.trainer import ICLConfig, ICLTrainer
    from icl_amd.utils.hashfill import synthetic_labels, synthetic_volume
    out = {}
    for rnd in range(2):                                   # the two configurations alternate: two rounds each
        for cin in (1, 4):
            torch.manual_seed(1337)
            model = unet_3D_icl(n_classes=2, in_channels=cin, device=dev)
            model.train()
            tr = ICLTrainer(model, ICLConfig(num_classes=2, labeled_bs=1), None)
            vol = synthetic_volume((2, cin, 96, 96, 96), 1337, device=dev)
            lab = synthetic_labels((1, 96, 96, 96), 4242, 2, device=dev)
            tr.capture(vol, lab, warmup=3)
            tr.step(vol, lab)
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(steps):
                last = tr.step(vol, lab)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t) / steps
            out.setdefault(f"in_channels_{cin}", []).append({"ms_per_step": round(dt * 1e3, 3), "loss": float(last["loss"])})
            del tr, model
            torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["feed", "conv", "step"])
    ap.add_argument("--launches", type=int, default=50, help="feed / conv: calls per timed window; step: timed steps")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("multimodal_time.py needs a HIP device")
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), a.what: {"feed": feed, "conv": conv, "step": step}[a.what](dev, a.launches)}
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
