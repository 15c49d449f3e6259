"""Measurements behind gradient clipping by the global norm (icl_amd.optim.clip_grad_norm_, csrc/kernels/gradclip.h; profiles/gradclip.md).
Needs the MI355X; every measurement is a child process under its own time limit, and the driver stops at the first child that fails.

    python tools/gradclip_probe.py                      the kernels alone: the factored norm at 13,824^2 for 8 / 64 / 160 factor rows, the
                                                        dense sum of squares and the scale on 2^23 elements (34 MB), the finish
    python tools/gradclip_probe.py --steps              the clip inside a step of the 96^3 unet_3D_icl (nc = 2): launches and time of the
                                                        clip alone on the step's real gradients, then ms / step interleaved in one
                                                        process — AdamW unclipped / clipped, SGD with its update inside backward /
                                                        update_in_backward off / clipped — eager and replayed
    python tools/gradclip_probe.py --norms [--max-norm C]   total_norm of the first four AdamW steps, unclipped (and clipped at C)
    python tools/gradclip_probe.py --band DIR --max-norm C  the band N of tests/test_gpu_gradclip.py: four steps of the trainer with
                                                        torch.optim.AdamW + torch.nn.utils.clip_grad_norm_(C) on dense gradients under
                                                        ICL_CONV_SPLIT=1 and =0, one process each, the clipping FusedAdamW trainer in a
                                                        third; rms differences per tensor (tensors travel through DIR)
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from adamw_probe import ADAMW, BAND_TENSORS, COPY_TBS, batch, build_trainer, timed  # noqa: E402

N = K = 13824
ROWS = (8, 64, 160)


def one_kernels():
    import torch
    from icl_amd import _lib
    L, dev = _lib.lib(), torch.device("cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    clip = torch.zeros(2, device=dev)
    for rows in ROWS:
        g, x = torch.randn(rows, N, device=dev) * 1e-2, torch.randn(rows, K, device=dev)
        nb, parts = L.icl_gradclip_factored_ws_bytes(rows, N, K), L.icl_gradclip_factored_parts(rows)
        ws, partial = torch.empty(nb // 8, dtype=torch.float64, device=dev), torch.empty(parts, dtype=torch.float64, device=dev)
        us = timed(lambda: _lib.check(L.icl_gradclip_sumsq_factored(g.data_ptr(), x.data_ptr(), rows, N, K, ws.data_ptr(), partial.data_ptr(),
                                                                    st), "factored"), reps=50)
        _lib.check(L.icl_gradclip_finish(partial.data_ptr(), parts, 1.0, clip.data_ptr(), st), "finish")
        ref = float((g.double().t() @ x.double()).pow(2).sum().sqrt()) if rows <= 64 else float("nan")
        print(f"rows {rows:4d}: factored norm (Gram + combine, 2 launches) {us:8.1f} us, reads {4e-6 * rows * (N + K):.2f} MB of factors, "
              f"{nb / 1e6:.2f} MB of slab partials, {rows * (rows + 1) * (N + K) / us / 1e6:6.2f} TFLOP/s fp64;  norm {float(clip[0])!r} "
              f"(fp64 multiplied out: {ref!r})", flush=True)
        del g, x, ws
    n = 1 << 23
    t = torch.randn(n, device=dev) * 1e-2
    chunks = 1024
    partial = torch.empty(chunks, dtype=torch.float64, device=dev)
    one, n64 = (ctypes.c_void_p * 1)(t.data_ptr()), (ctypes.c_int64 * 1)(n)
    us = timed(lambda: _lib.check(L.icl_gradclip_sumsq(one, n64, 1, chunks, partial.data_ptr(), st), "sumsq"), reps=50)
    print(f"dense sum of squares 2^23 (34 MB, cache-resident): {us:8.1f} us  {4.0 * n / us / 1e6:5.2f} TB/s "
          f"({4.0 * n / COPY_TBS / 1e6:.1f} us at the {COPY_TBS} TB/s copy rate)", flush=True)
    us = timed(lambda: _lib.check(L.icl_gradclip_finish(partial.data_ptr(), chunks, 1e-3, clip.data_ptr(), st), "finish"), reps=50)
    print(f"finish over {chunks} partial sums: {us:8.1f} us;  coef {float(clip[1])!r}", flush=True)
    for coef in (0.5, 1.0):
        clip[1] = coef
        us = timed(lambda: _lib.check(L.icl_gradclip_scale(one, one, n64, 1, chunks, clip.data_ptr(), st), "scale"), reps=50)
        print(f"scale in place 2^23, coef {coef}: {us:8.1f} us  {8.0 * n / us / 1e6:5.2f} TB/s of 8 B / element", flush=True)


def one_clip_alone():
    """The clip on the real gradients of one step: launches by entry point and event time of the whole eager sequence."""
    import torch
    from icl_amd import _lib, optim
    vol, lab = batch()
    model, tr = build_trainer(dict(ADAMW, max_grad_norm=1e30), max_iterations=30000)
    tr.step(vol, lab)
    tr._forward_backward(vol, lab)
    params = [p for g in tr.optimizer.param_groups for p in g["params"]]
    dense = [p.grad for p in params if p.grad is not None]
    fac = [p._icl_factors for p in params if getattr(p, "_icl_factors", None)]
    print(f"gradients of one step: {len(dense)} dense tensors, {sum(g.numel() for g in dense) * 4e-6:.1f} MB, "
          f"{sum(1 for g in dense if g.numel() >= optim._BIG)} of them >= 2^20 elements; {len(fac)} factored weights with "
          f"{[sum(f[0].shape[0] for f in fs) for fs in fac]} rows", flush=True)
    L = _lib.lib()
    counts = {}
    orig = {n: getattr(L, n) for n in optim._CLIP_ENTRIES}
    for n in orig:
        def wrap(*a, _n=n):
            counts[_n] = counts.get(_n, 0) + 1
            return orig[_n](*a)
        setattr(L, n, wrap)
    optim._clip_gradients(params, 1e30, tr.optimizer._clip)
    for n in orig:
        setattr(L, n, orig[n])
    print("entry-point calls of one clip:", counts, flush=True)
    for c in (1e30, 1e-3):
        us = timed(lambda: optim._clip_gradients(params, c, tr.optimizer._clip), reps=20)
        print(f"clip alone, eager launches, max_norm {c:g}: {us:8.1f} us (norm {float(tr.optimizer._clip.clip_dev[0])!r}, "
              f"coef {float(tr.optimizer._clip.clip_dev[1])!r})", flush=True)
    tr.optimizer.abandon_step()


def one_steps():
    import time
    import torch
    vol, lab = batch()
    sgd = dict(base_lr=0.01)
    configs = {"adamw": ADAMW, "adamw+clip": dict(ADAMW, max_grad_norm=1.0), "sgd": sgd, "sgd, update_in_backward off": dict(sgd, update_in_backward=False),
               "sgd+clip": dict(sgd, max_grad_norm=1.0)}
    trainers = {k: build_trainer(v, max_iterations=30000)[1] for k, v in configs.items()}

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
            print(phase, rnd, "  ".join(f"{name} {ms(tr, 10):7.3f}" for name, tr in trainers.items()), "ms/step", flush=True)


def one_norms(max_norm):
    vol, lab = batch()
    for c in [1e30] + ([max_norm] if max_norm else []):
        model, tr = build_trainer(dict(ADAMW, max_grad_norm=c))
        out = []
        for _ in range(4):
            r = tr.step(vol, lab)
            out.append((float(r["loss"]), float(r["grad_norm"]), float(tr.optimizer.clip_dev[1])))
        print(f"max_grad_norm {c:g}: (loss, total_norm, coef) of steps 1..4:", out, flush=True)
        del model, tr


def band_run(kind, out_dir, max_norm):
    """kind: "ref" (torch.optim.AdamW + torch's clip, dense gradients; ICL_CONV_SPLIT from the environment) or "fused"."""
    import torch
    vol, lab = batch()
    norms = []
    if kind == "ref":
        model, tr = build_trainer(ADAMW, factored=False)
        opt = torch.optim.AdamW(model.parameters(), lr=ADAMW["base_lr"], betas=(0.9, 0.999), eps=1e-8, weight_decay=ADAMW["weight_decay"],
                                foreach=False)

        class Clipped:      # torch's clip between backward and step, where the reference recipe has it
            param_groups = opt.param_groups

            def zero_grad(self, set_to_none=True):
                opt.zero_grad(set_to_none=set_to_none)

            def step(self):
                norms.append(float(torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm)))
                opt.step()

            def abandon_step(self):
                pass
        tr.optimizer = Clipped()
    else:
        model, tr = build_trainer(dict(ADAMW, max_grad_norm=max_norm))
    losses = []
    for _ in range(4):
        r = tr.step(vol, lab)
        losses.append(float(r["loss"]))
        if kind != "ref":
            norms.append(float(r["grad_norm"]))
    p = dict(model.named_parameters())
    torch.save({"losses": losses, "norms": norms, **{k: p[k].detach().cpu() for k in BAND_TENSORS}},
               os.path.join(out_dir, f"band_{kind}_{os.environ.get('ICL_CONV_SPLIT', '1')}.pt"))
    print(kind, os.environ.get("ICL_CONV_SPLIT", "1"), "losses", losses, "norms", norms, flush=True)


def band_compare(out_dir):
    import torch

    def rms(a, b):
        a, b = a.double(), b.double()
        return float(((a - b) ** 2).mean().sqrt() / (b ** 2).mean().sqrt())
    r1, r0, fu = (torch.load(os.path.join(out_dir, f)) for f in ("band_ref_1.pt", "band_ref_0.pt", "band_fused_1.pt"))
    out = {"N": {}, "fused_vs_ref": {}}
    for k in BAND_TENSORS:
        out["N"][k], out["fused_vs_ref"][k] = rms(r0[k], r1[k]), rms(fu[k], r1[k])
    for what in ("losses", "norms"):
        out["N"][what] = [abs(a - b) / abs(b) for a, b in zip(r0[what], r1[what])]
        out["fused_vs_ref"][what] = [abs(a - b) / abs(b) for a, b in zip(fu[what], r1[what])]
    out["losses_ref"], out["norms_ref"] = r1["losses"], r1["norms"]
    print(json.dumps(out, indent=1), flush=True)


def child(args, limit, env=None):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__)] + args
    print("+", " ".join(cmd[4:]), flush=True)
    rc = subprocess.run(cmd, env={**os.environ, **(env or {})}).returncode
    if rc != 0:
        sys.exit(f"gradclip_probe: {' '.join(args)} ended with {rc}; nothing further is started")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", action="store_true")
    ap.add_argument("--norms", action="store_true")
    ap.add_argument("--band", metavar="DIR")
    ap.add_argument("--max-norm", type=float, default=None)
    ap.add_argument("--one", help=argparse.SUPPRESS)
    a = ap.parse_args()
    mn = [] if a.max_norm is None else ["--max-norm", repr(a.max_norm)]
    if a.one:
        kind, _, arg = a.one.partition(":")
        {"kernels": one_kernels, "clip_alone": one_clip_alone, "steps": one_steps, "norms": lambda: one_norms(a.max_norm),
         "band_ref": lambda: band_run("ref", arg, a.max_norm), "band_fused": lambda: band_run("fused", arg, a.max_norm),
         "band_compare": lambda: band_compare(arg)}[kind]()
    elif a.steps:
        child(["--one", "clip_alone"], 240)
        child(["--one", "steps"], 540)
    elif a.norms:
        child(["--one", "norms"] + mn, 300)
    elif a.band:
        if a.max_norm is None:
            sys.exit("--band needs --max-norm")
        os.makedirs(a.band, exist_ok=True)
        child(["--one", f"band_ref:{a.band}"] + mn, 300, {"ICL_CONV_SPLIT": "1"})
        child(["--one", f"band_ref:{a.band}"] + mn, 300, {"ICL_CONV_SPLIT": "0"})
        child(["--one", f"band_fused:{a.band}"] + mn, 300, {"ICL_CONV_SPLIT": "1"})
        child(["--one", f"band_compare:{a.band}"], 120)
    else:
        child(["--one", "kernels"], 240)


if __name__ == "__main__":
    main()
