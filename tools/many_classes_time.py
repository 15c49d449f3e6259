"""Times of the loss and prototype-attention kernels across the 16-class boundary, on the MI355X -> profiles/many_classes_time.json.

usage (GPU box, from the repository root):  python tools/many_classes_time.py [--reps 20] [--out profiles/many_classes_time.json]

Losses, [2, nc, 96, 96, 96] logits, forward (statistics + finalize) and backward (gradient) of one term:
  mode 1 (cross-entropy + Dice on labels) and mode 3 (soft-max MSE against a second logit tensor)
  nc = 16 on the register path and, with ICL_LOSS_GENERIC=1, on the generic-class path; nc = 40 on the generic-class path
Prototype attention at the 24^3 level (13,824 tokens, batch 2, 4 heads of 16): forward (logits + soft-max.V) and backward with the dQ-share
workspace, nc = 16 (one class tile) and nc = 40 (three tiles).
Every figure is the median (min, max) over --reps device-event timings after two warm-up calls, in one process; a call is a handful of
launches, so launch gaps are part of it.  Kernel-by-kernel times: run it under `rocprofv3 --kernel-trace --stats` in a separate call.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from icl_amd import ops  # noqa: E402
from icl_amd.utils.hashfill import synthetic_labels, synthetic_volume  # noqa: E402


def timed(fn, reps):
    for _ in range(2):
        fn()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4))


def loss_case(dev, nc, mode, generic, reps):
    if generic:
        os.environ["ICL_LOSS_GENERIC"] = "1"
    else:
        os.environ.pop("ICL_LOSS_GENERIC", None)
    shape = (2, nc, 96, 96, 96)
    a = torch.cat([synthetic_volume((1,) + shape[1:], 3 + i) for i in range(2)]).to(dev).requires_grad_()
    tgt = synthetic_labels((2, 96, 96, 96), 5, nc).to(dev) if mode == 1 else a.detach().flip(1).contiguous()
    out = {}
    state = {}

    def fwd():
        state["pair"] = ops._FusedLoss.apply(a, tgt, None, mode, False)

    def bwd():
        a.grad = None
        p = state["pair"]
        (p[0] + p[1]).backward(retain_graph=True) if mode == 1 else p[0].backward(retain_graph=True)

    out["fwd"] = timed(fwd, reps)
    out["bwd"] = timed(bwd, reps)
    os.environ.pop("ICL_LOSS_GENERIC", None)
    return out


def attn_case(dev, nc, reps, B=2, h=4, d=16, N=13824):
    qh = synthetic_volume((B, h, nc, d), 7).to(dev).requires_grad_()
    kv = synthetic_volume((B, N, 2 * h * d), 8).to(dev).requires_grad_()
    go, gl = synthetic_volume((B, h, nc, d), 9).to(dev), synthetic_volume((B, nc, h, N), 10).to(dev)
    state = {}

    def fwd():
        state["o"] = ops.prototype_attention(qh, kv, h, d ** -0.5)

    def bwd():
        qh.grad = kv.grad = None
        torch.autograd.backward(state["o"], (go, gl), retain_graph=True)

    return dict(fwd=timed(fwd, reps), bwd=timed(bwd, reps))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "many_classes_time.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "loss": {}, "attention": {}}
    for nc, generic in ((16, False), (16, True), (40, True)):
        for mode in (1, 3):
            key = f"nc{nc}_mode{mode}_{'generic' if generic else 'register'}"
            res["loss"][key] = loss_case(dev, nc, mode, generic, args.reps)
            print(key, res["loss"][key], flush=True)
            torch.cuda.empty_cache()
    for nc in (16, 40):
        res["attention"][f"nc{nc}"] = attn_case(dev, nc, args.reps)
        print("attention", nc, res["attention"][f"nc{nc}"], flush=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)
