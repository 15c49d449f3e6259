"""Time the AMOS cached prefix on the MI355X (icl_prefix_box + icl_prefix_resample through amos_prefix) beside the alternative a user
would otherwise write on the same device and data: the window in torch, then F.grid_sample twice -> profiles/amos_prefix.json.

usage (GPU box, from the repository root):  python tools/amos_prefix_time.py [--out profiles/amos_prefix.json]

One realistic case, raw 512 x 512 x 120 at (0.78, 0.78, 5.0) -> (267, 267, 298) (foreground on every face: nothing is cropped), the raw
pair resident on the device.  A timed window is LAUNCHES = 12 calls between two device events, each call on the next of SETS = 4 copies
of the inputs and outputs (157 MB raw + 106 MB out a set: a call's data was last touched three calls and more than 750 MB ago, beyond
the 256 MB last-level cache), so one launch's latency is not the figure and no call rereads what the one before left in a cache.  A
figure is the window's time over LAUNCHES; warm-up of 3 windows, median of 10:
  prefix_ms         amos_prefix on device tensors: both box launches, the read-back of the six integers, the resample launch
  box_ms            icl_prefix_box alone            bytes: the raw image once (4 B a voxel)
  resample_ms       icl_prefix_resample alone       bytes: the raw image and label once (5 B a raw voxel), both outputs (5 B an output voxel)
  permuted_ms       icl_prefix_resample with oriented axis 2 = raw axis 0 (strided reads), same raw volumes
  torch_ms          (v - a_min) / range clamped, then grid_sample bilinear (image) and nearest (label as fp32), grid prebuilt outside the window
  copy_gbps         dst.copy_(src) of 512 MiB of fp32 over rotating pairs: the copy rate this machine reaches (bytes read + written over time)
  *_fraction        bytes / time over copy_gbps
  *_single_ms       the same call alone in its window on ONE set (launch latency inside, inputs possibly cached): for comparison only
The torch result is compared with the prefix (max abs difference of the image, mismatching label voxels), and the permuted output with
the aligned one transposed back, and both are reported, not asserted.  No threshold is asserted: this tool only records.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from icl_amd import _lib  # noqa: E402
from icl_amd.dataloaders.amos import PREFIX_BOX_WS_INTS, amos_prefix, plan_prefix  # noqa: E402

RAW = (512, 512, 120)
SPACING = (0.78, 0.78, 5.0)
SETS, LAUNCHES = 4, 12
WARMUP, TIMED = 3, 10


def timed(call, launches=LAUNCHES):
    """``call(k)`` runs the work on buffer set ``k % SETS``; returns (median, minimum) milliseconds per call."""
    times = []
    for n in range(WARMUP + TIMED):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for k in range(launches):
            call(k)
        e1.record()
        torch.cuda.synchronize()
        if n >= WARMUP:
            times.append(e0.elapsed_time(e1) / launches)
    return statistics.median(times), min(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "amos_prefix.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("amos_prefix_time.py needs a HIP device")
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(2022)
    image = (torch.rand(RAW, generator=g) * 1400.0 - 1000.0)                       # Hounsfield-like: two fifths above the window's floor
    image[0, 0, 0] = image[-1, -1, -1] = 100.0                                      # foreground on every face
    label = torch.randint(0, 16, RAW, generator=g, dtype=torch.uint8)
    images = [image.to(dev) for _ in range(SETS)]
    labels = [label.to(dev) for _ in range(SETS)]
    L = _lib.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream

    image_t, label_t, plan = amos_prefix(images[0], labels[0], dev, spacing=SPACING, axcodes="RAS")
    assert plan.out_shape == (267, 267, 298), plan
    out_i = [image_t] + [torch.empty_like(image_t) for _ in range(SETS - 1)]
    out_l = [label_t] + [torch.empty_like(label_t) for _ in range(SETS - 1)]
    res = {"device": torch.cuda.get_device_name(0), "raw": list(RAW), "spacing": list(SPACING), "out": list(plan.out_shape),
           "sets": SETS, "launches_per_window": LAUNCHES, "warmup": WARMUP, "timed": TIMED}
    raw_voxels, out_voxels = int(np.prod(RAW)), int(np.prod(plan.out_shape))

    def whole(k):
        k %= SETS
        amos_prefix(images[k], labels[k], dev, spacing=SPACING, axcodes="RAS", out=(out_i[k], out_l[k]))

    res["prefix_ms"], res["prefix_ms_min"] = timed(whole)
    res["prefix_single_ms"], _ = timed(lambda k: whole(0), launches=1)

    box, ws = torch.empty(6, dtype=torch.int32, device=dev), torch.empty(PREFIX_BOX_WS_INTS, dtype=torch.int32, device=dev)
    window = plan.window_params()

    def find_box(k):
        _lib.check(L.icl_prefix_box(images[k % SETS].data_ptr(), *RAW, window, 1, box.data_ptr(), ws.data_ptr(), stream))

    res["box_ms"], res["box_ms_min"] = timed(find_box)
    res["box_single_ms"], _ = timed(lambda k: find_box(0), launches=1)
    res["box_bytes"] = 4 * raw_voxels

    def resample(p, oi, ol):
        ints, doubles = p.int_params(), p.double_params()

        def call(k):
            k %= SETS
            _lib.check(L.icl_prefix_resample(images[k].data_ptr(), labels[k].data_ptr(), ints, doubles, window, 1, oi[k].data_ptr(),
                                             ol[k].data_ptr(), stream))
        return call

    call = resample(plan, out_i, out_l)
    res["resample_ms"], res["resample_ms_min"] = timed(call)
    res["resample_single_ms"], _ = timed(lambda k: call(0), launches=1)
    res["resample_bytes"] = 5 * raw_voxels + 5 * out_voxels

    # oriented axis 2 = raw axis 0: "SRA" (source axis 0 runs up), the raw spacing permuted so that the oriented one is SPACING again.
    # Output (267, 63, 1278): three tiles along oriented axis 2.  Its content is checked against the literal numpy chain for other
    # shapes in the tests; here it is compared with what the aligned orientation gives for the transposed raw pair.
    permuted = plan_prefix(RAW, plan.box, spacing=(SPACING[2], SPACING[0], SPACING[1]), axcodes="SRA")
    pi = [torch.empty(permuted.out_shape, dtype=torch.float32, device=dev) for _ in range(SETS)]
    pl = [torch.empty(permuted.out_shape, dtype=torch.uint8, device=dev) for _ in range(SETS)]
    res["permuted_perm"], res["permuted_out"] = list(permuted.perm), list(permuted.out_shape)
    call = resample(permuted, pi, pl)
    res["permuted_ms"], res["permuted_ms_min"] = timed(call)
    res["permuted_single_ms"], _ = timed(lambda k: call(0), launches=1)
    res["permuted_bytes"] = 5 * raw_voxels + 5 * int(np.prod(permuted.out_shape))
    straight_i, straight_l, straight = amos_prefix(images[0].permute(1, 2, 0).contiguous(), labels[0].permute(1, 2, 0).contiguous(), dev,
                                                   spacing=(SPACING[0], SPACING[1], SPACING[2]), axcodes="RAS")
    res["permuted_equals_transposed_input"] = bool(straight.out_shape == permuted.out_shape and torch.equal(straight_i, pi[0])
                                                   and torch.equal(straight_l, pl[0]))
    del straight_i, straight_l

    # the alternative: torch on the same device and data
    coords = [torch.clamp(torch.arange(o, dtype=torch.float64) * (p / s), 0, m - 1) * (2.0 / (m - 1)) - 1.0
              for o, m, s, p in zip(plan.out_shape, plan.padded_shape, plan.spacing, plan.pixdim)]
    g0, g1, g2 = torch.meshgrid(*coords, indexing="ij")
    grid = torch.stack([g2, g1, g0], dim=-1).to(torch.float32)[None].to(dev)
    a_min, a_range = plan.window[0], plan.window[1]
    held = {}

    def with_torch(k):
        k %= SETS
        w = torch.clamp((images[k] - a_min) / a_range, 0.0, 1.0)
        held["image"] = F.grid_sample(w[None, None], grid, mode="bilinear", padding_mode="border", align_corners=True)
        held["label"] = F.grid_sample(labels[k].to(torch.float32)[None, None], grid, mode="nearest", padding_mode="border",
                                      align_corners=True).to(torch.uint8)

    res["torch_ms"], res["torch_ms_min"] = timed(with_torch)
    res["torch_grid_bytes"] = grid.numel() * 4
    res["torch_image_max_abs_diff"] = float((held["image"][0, 0] - image_t).abs().max())
    res["torch_label_mismatches"] = int((held["label"][0, 0] != label_t).sum())
    del held, grid

    n = 128 * 1024 * 1024
    srcs = [torch.empty(n, dtype=torch.float32, device=dev).normal_() for _ in range(2)]
    dsts = [torch.empty(n, dtype=torch.float32, device=dev) for _ in range(2)]
    copy_ms, _ = timed(lambda k: dsts[k % 2].copy_(srcs[k % 2]))
    res["copy_gbps"] = 2 * 4 * n / (copy_ms * 1e-3) / 1e9
    for key in ("box", "resample", "permuted"):
        res[f"{key}_gbps"] = res[f"{key}_bytes"] / (res[f"{key}_ms"] * 1e-3) / 1e9
        res[f"{key}_fraction"] = res[f"{key}_gbps"] / res["copy_gbps"]
    res = {k: (float(f"{v:.5g}") if isinstance(v, float) else v) for k, v in res.items()}
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
