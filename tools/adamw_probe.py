"""Measurements behind icl_amd.optim.FusedAdamW (profiles/adamw.md).  Needs the MI355X; every measurement is a child process under its
own time limit, and the driver stops at the first child that fails.

    python tools/adamw_probe.py                  the three kernels: adamw_factored_kernel at 13,824^2 for several factor row counts beside
                                                 the multiplied-out alternative (ops._tall_atb + adamw_kernel), adamw_kernel on 2^24
                                                 elements, adamw_multi_kernel on 48 small tensors
    python tools/adamw_probe.py --steps          ms / step of ICLTrainer(optimizer="adamw") and of the SGD trainer, eager and replayed,
                                                 interleaved in one process (96^3 unet_3D_icl, nc = 2)
    python tools/adamw_probe.py --band DIR       the band N of tests/test_gpu_adamw.py: four steps of the trainer with torch.optim.AdamW
                                                 and dense gradients under ICL_CONV_SPLIT=1 and =0, one process each, the FusedAdamW trainer
                                                 in a third; rms differences per tensor (tensors travel through DIR)
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = K = 13824
ROWS = (8, 32, 64, 128, 192, 256, 384)
COPY_TBS = 6.29          # measured float4 copy rate of the MI355X (micro-architecture guide)
BAND_TENSORS = ("final.weight", "sspa.class_decoders.2.mlp2.fc1.weight", "sspa.class_decoders.2.norm2.bias")


def timed(fn, reps=10, warm=3):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3      # microseconds


def hyper():
    from icl_amd.optim import adamw_scalars
    return adamw_scalars(1e-3, 1e-2, 0.9, 0.999, 1e-8, 10.0)


def one_factored():
    import torch
    from icl_amd import _lib, ops
    L, dev = _lib.lib(), torch.device("cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = torch.randn(N, K, device=dev) * 0.05
    m, v = torch.zeros_like(p), torch.full_like(p, 1e-4)
    sc = hyper()
    dense_g = torch.randn(N, K, device=dev) * 1e-2

    def dense():
        _lib.check(L.icl_adamw_step(p.data_ptr(), dense_g.data_ptr(), m.data_ptr(), v.data_ptr(), N * K, *sc, 0, None, st), "adamw")
    us = timed(dense)
    print(f"adamw_kernel 13,824^2: {us:8.1f} us  {28.0 * N * K / us / 1e6:5.2f} TB/s of the 28 B / parameter floor "
          f"({28.0 * N * K / COPY_TBS / 1e6:.0f} us at the {COPY_TBS} TB/s copy rate)", flush=True)
    del dense_g
    for rows in ROWS:
        g, x = torch.randn(rows, N, device=dev) * 1e-2, torch.randn(rows, K, device=dev)

        def factored():
            _lib.check(L.icl_adamw_step_factored(p.data_ptr(), m.data_ptr(), v.data_ptr(), g.data_ptr(), x.data_ptr(), rows, N, K, *sc, 0,
                                                 None, st), "adamw factored")

        def multiplied_out():
            d = ops._tall_atb(g, x, False)[0]
            _lib.check(L.icl_adamw_step(p.data_ptr(), d.data_ptr(), m.data_ptr(), v.data_ptr(), N * K, *sc, 0, None, st), "adamw")
        uf, um = timed(factored), timed(multiplied_out)
        print(f"rows {rows:4d}: adamw_factored_kernel {uf:8.1f} us  {24.0 * N * K / uf / 1e6:5.2f} TB/s of the 24 B / weight floor "
              f"({24.0 * N * K / COPY_TBS / 1e6:.0f} us at copy rate), {2.0 * rows * N * K / uf / 1e6:6.1f} TFLOP/s   |   _tall_atb + adamw_kernel "
              f"{um:8.1f} us", flush=True)


def one_dense():
    import torch
    from icl_amd import _lib
    L, dev = _lib.lib(), torch.device("cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    n = 1 << 24
    p, g = torch.randn(n, device=dev) * 0.05, torch.randn(n, device=dev) * 1e-2
    m, v = torch.zeros_like(p), torch.full_like(p, 1e-4)
    sc = hyper()
    us = timed(lambda: _lib.check(L.icl_adamw_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, *sc, 0, None, st), "adamw"), reps=50)
    print(f"adamw_kernel 2^24: {us:8.1f} us  {28.0 * n / us / 1e6:5.2f} TB/s of the 28 B / parameter floor ({28.0 * n / COPY_TBS / 1e6:.0f} us at "
          f"copy rate; 470 MB: inside the 256 MB Infinity Cache only in part)", flush=True)
    # 48 tensors of 2^16 elements in one launch
    cnt, each = 48, 1 << 16
    arr = ctypes.c_void_p * cnt
    ptrs = [arr(*[t[i * each:].data_ptr() for i in range(cnt)]) for t in (p, g, m, v)]
    ns = (ctypes.c_int64 * cnt)(*[each] * cnt)
    us = timed(lambda: _lib.check(L.icl_adamw_step_multi(*ptrs, ns, cnt, *sc, 0, None, st), "adamw multi"), reps=50)
    print(f"adamw_multi_kernel 48 x 2^16: {us:8.1f} us  {28.0 * cnt * each / us / 1e6:5.2f} TB/s (88 MB: cache-resident, launch-shaped)", flush=True)


def build_trainer(optimizer, factored=True, max_iterations=10):
    import torch
    from icl_amd import ops
    from icl_amd.networks.aligner import DropPath
    from icl_amd.networks.layers import Dropout3
    from icl_amd.networks.unet_3D_icl import unet_3D_icl
    from icl_amd.trainer import ICLConfig, ICLTrainer
    from icl_amd.utils.hashfill import fill_like_reference_init
    dev = torch.device("cuda", 0)
    ops.StepRNG.tensor = None
    model = unet_3D_icl(n_classes=2, in_channels=1, device=dev)
    fill_like_reference_init(list(model.named_parameters()))
    for mod in model.modules():      # parity mode: no dropout, so that two runs differ by rounding only
        if isinstance(mod, Dropout3):
            mod.p = 0.0
        if isinstance(mod, DropPath):
            mod.drop_prob = 0.0
    model.train()
    cfg = ICLConfig(num_classes=2, labeled_bs=1, max_iterations=max_iterations, factored_mlp2_grads=factored, **optimizer)
    return model, ICLTrainer(model, cfg)


ADAMW = dict(optimizer="adamw", base_lr=1e-3, weight_decay=1e-2)


def batch():
    import torch
    from icl_amd.utils.hashfill import synthetic_labels, synthetic_volume
    dev = torch.device("cuda", 0)
    return synthetic_volume((2, 1, 96, 96, 96), 1337).to(dev), synthetic_labels((1, 96, 96, 96), 4242, 2).to(dev)


def one_steps():
    import time
    import torch
    vol, lab = batch()
    trainers = {"sgd": build_trainer({}, max_iterations=30000)[1], "adamw": build_trainer(ADAMW, max_iterations=30000)[1]}

    def ms(tr, reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            tr.step(vol, lab)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps * 1e3
    for phase in ("eager", "replayed"):
        for name, tr in trainers.items():
            if phase == "replayed":
                tr.capture(vol, lab, warmup=2)
            ms(tr, 3)
        for rnd in range(3):      # interleaved
            print(phase, rnd, "  ".join(f"{name} {ms(tr, 10):7.3f} ms/step" for name, tr in trainers.items()), flush=True)


def band_run(kind, out_dir):
    """kind: "ref" (torch.optim.AdamW, dense gradients; ICL_CONV_SPLIT from the environment) or "fused" (FusedAdamW, factored)."""
    import torch
    vol, lab = batch()
    model, tr = build_trainer(ADAMW, factored=(kind == "fused"))
    if kind == "ref":
        tr.optimizer = torch.optim.AdamW(model.parameters(), lr=ADAMW["base_lr"], betas=(0.9, 0.999), eps=1e-8,
                                         weight_decay=ADAMW["weight_decay"], foreach=False)
    losses = [float(tr.step(vol, lab)["loss"]) for _ in range(4)]
    p = dict(model.named_parameters())
    torch.save({"losses": losses, **{k: p[k].detach().cpu() for k in BAND_TENSORS}}, os.path.join(out_dir, f"band_{kind}_{os.environ.get('ICL_CONV_SPLIT', '1')}.pt"))
    print(kind, os.environ.get("ICL_CONV_SPLIT", "1"), losses, flush=True)


def band_compare(out_dir):
    import torch

    def rms(a, b):
        a, b = a.double(), b.double()
        return float(((a - b) ** 2).mean().sqrt() / (b ** 2).mean().sqrt())
    r1, r0, fu = (torch.load(os.path.join(out_dir, f)) for f in ("band_ref_1.pt", "band_ref_0.pt", "band_fused_1.pt"))
    out = {"N": {}, "fused_vs_ref": {}}
    for k in BAND_TENSORS:
        out["N"][k], out["fused_vs_ref"][k] = rms(r0[k], r1[k]), rms(fu[k], r1[k])
    out["N"]["losses"] = [abs(a - b) / abs(b) for a, b in zip(r0["losses"], r1["losses"])]
    out["fused_vs_ref"]["losses"] = [abs(a - b) / abs(b) for a, b in zip(fu["losses"], r1["losses"])]
    out["losses_ref"] = r1["losses"]
    print(json.dumps(out, indent=1), flush=True)


def child(args, limit, env=None):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__)] + args
    print("+", " ".join(cmd[4:]), flush=True)
    rc = subprocess.run(cmd, env={**os.environ, **(env or {})}).returncode
    if rc != 0:
        sys.exit(f"adamw_probe: {' '.join(args)} ended with {rc}; nothing further is started")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", action="store_true")
    ap.add_argument("--band", metavar="DIR")
    ap.add_argument("--one", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        kind, _, arg = a.one.partition(":")
        {"factored": one_factored, "dense": one_dense, "steps": one_steps, "band_ref": lambda: band_run("ref", arg),
         "band_fused": lambda: band_run("fused", arg), "band_compare": lambda: band_compare(arg)}[kind]()
    elif a.steps:
        child(["--one", "steps"], 420)
    elif a.band:
        os.makedirs(a.band, exist_ok=True)
        child(["--one", f"band_ref:{a.band}"], 300, {"ICL_CONV_SPLIT": "1"})
        child(["--one", f"band_ref:{a.band}"], 300, {"ICL_CONV_SPLIT": "0"})
        child(["--one", f"band_fused:{a.band}"], 300, {"ICL_CONV_SPLIT": "1"})
        child(["--one", f"band_compare:{a.band}"], 120)
    else:
        child(["--one", "factored"], 180)
        child(["--one", "dense"], 120)


if __name__ == "__main__":
    main()
