"""Measurements behind the voxel-wise loss kernels (csrc/kernels/loss_point.h: softmax KL, entropy, focal; profiles/point_losses.md).
Needs the MI355X; every measurement is a child process under its own time limit, and the driver stops at the first child that fails.

    python tools/point_loss_probe.py                     each entry point, forward and backward, at [2, 2, 96^3] and [2, 16, 96^3] with
                                                         events, and the torch composition of the same formula interleaved in the same
                                                         process (the baseline: no such operator existed before); bytes moved and the
                                                         fraction of the copy rate; three rounds, median and spread
    python tools/point_loss_probe.py --band              the N of tests/point_loss_ref.py's LARGE_N: the error of the plain torch fp32
                                                         evaluation against the fp64 restatement at the two grid-stride wrap-around
                                                         shapes, beside the kernels' own error
    python tools/point_loss_probe.py --trainer-band DIR  the band N of tests/test_gpu_point_loss.py: four steps of the 96^3 unet_3D_icl
                                                         trainer with consistency="kl", w_ent=0.1 and torch.optim.SGD on dense gradients
                                                         under ICL_CONV_SPLIT=1 and =0, one process each; the fused trainer eager and
                                                         captured in two more; rms differences per tensor (tensors travel through DIR)
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from adamw_probe import BAND_TENSORS, COPY_TBS, batch, build_trainer, timed  # noqa: E402

OPTIONS = dict(consistency="kl", w_ent=0.1)
SGD = dict(lr=0.01, momentum=0.9, weight_decay=1e-4)      # ICLConfig's defaults


# ---- the kernels alone ------------------------------------------------------------------------------------------------------------------------

def torch_kl(a, b):
    la, lb = torch_log_softmax(a), torch_log_softmax(b)
    return 0.5 * (lb.exp() * (lb - la)).mean() + 0.5 * (la.exp() * (la - lb)).mean()


def torch_log_softmax(x):
    import torch
    return torch.log_softmax(x, 1)


def torch_entropy(x):
    import torch
    p = torch.softmax(x, 1)
    return -(p * torch.log(p + 1e-6)).sum(1).mean()


def torch_focal(x, y, alpha, gamma=1.5):
    import torch
    logpt = torch.log_softmax(x, 1).gather(1, y[:, None])[:, 0]
    pt = logpt.detach().exp()
    return (-alpha[y] * (1 - pt) ** gamma * logpt).mean()


def one_kernels():
    import torch
    from icl_amd import _lib, ops
    from icl_amd.utils.hashfill import synthetic_labels
    L, dev = _lib.lib(), torch.device("cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    ws, out, g = torch.empty(ops.LOSS_MAX_BLOCKS, device=dev), torch.empty(1, device=dev), torch.full((1,), 1.3, device=dev)
    for nc in (2, 16):
        shape = (2, nc, 96, 96, 96)
        V = 2 * 96 ** 3
        a, b = torch.randn(shape, device=dev) * 2, torch.randn(shape, device=dev) * 2
        y = synthetic_labels((2, 96, 96, 96), 4242, nc).to(dev)
        alpha = torch.linspace(0.2, 0.8, nc, device=dev)
        ga, gb = torch.empty_like(a), torch.empty_like(b)
        geo = (2, nc, 96 ** 3)
        T = 4.0 * nc * V       # bytes of one [2, nc, 96^3] fp32 tensor
        ar, br = a.clone().requires_grad_(), b.clone().requires_grad_()

        def fb(fn, *inputs):      # the torch composition: forward alone, then forward + backward
            def fwd():
                with torch.no_grad():
                    fn(*inputs)

            def both():
                for t in inputs:
                    if t.is_floating_point() and t.requires_grad:
                        t.grad = None
                (fn(*inputs) * 1.3).backward()
            return fwd, both
        rows = [
            ("kl fwd", 2 * T, lambda: L.icl_kl_fwd(P(a), P(b), P(ws), P(out), *geo, 0.5, 0.5, st), fb(torch_kl, ar, br)[0]),
            ("kl bwd (ga, gb)", 4 * T, lambda: L.icl_kl_bwd(P(a), P(b), P(g), P(ga), P(gb), *geo, 0.5, 0.5, st), None),
            ("kl bwd (ga)", 3 * T, lambda: L.icl_kl_bwd(P(a), P(b), P(g), P(ga), None, *geo, 0.5, 0.5, st), None),
            ("kl fwd + bwd (ga, gb)", 6 * T, lambda: (L.icl_kl_fwd(P(a), P(b), P(ws), P(out), *geo, 0.5, 0.5, st),
                                                     L.icl_kl_bwd(P(a), P(b), P(g), P(ga), P(gb), *geo, 0.5, 0.5, st)), fb(torch_kl, ar, br)[1]),
            ("entropy(from_logits) fwd", T, lambda: L.icl_entropy_fwd(P(a), P(ws), P(out), None, *geo, 1, 1.0, st), fb(torch_entropy, ar)[0]),
            ("entropy(from_logits) bwd", 2 * T, lambda: L.icl_entropy_bwd(P(a), P(g), None, P(ga), *geo, 1, 1.0, st), None),
            ("entropy fwd + bwd", 3 * T, lambda: (L.icl_entropy_fwd(P(a), P(ws), P(out), None, *geo, 1, 1.0, st),
                                                 L.icl_entropy_bwd(P(a), P(g), None, P(ga), *geo, 1, 1.0, st)), fb(torch_entropy, ar)[1]),
            ("focal fwd", T + 8.0 * V, lambda: L.icl_focal_fwd(P(a), P(y), P(alpha), P(ws), P(out), *geo, 1.5, 1, st),
             fb(torch_focal, ar, y, alpha)[0]),
            ("focal bwd", 2 * T + 8.0 * V, lambda: L.icl_focal_bwd(P(a), P(y), P(alpha), P(g), P(ga), *geo, 1.5, 1, st), None),
            ("focal fwd + bwd", 3 * T + 16.0 * V, lambda: (L.icl_focal_fwd(P(a), P(y), P(alpha), P(ws), P(out), *geo, 1.5, 1, st),
                                                          L.icl_focal_bwd(P(a), P(y), P(alpha), P(g), P(ga), *geo, 1.5, 1, st)),
             fb(torch_focal, ar, y, alpha)[1]),
        ]
        print(f"[2, {nc}, 96^3]: one tensor is {T / 1e6:.1f} MB; copy rate {COPY_TBS} TB/s", flush=True)
        for name, nbytes, mine, theirs in rows:
            r = mine()
            assert r == 0 or r == (0, 0), (name, L.icl_last_error())
            mine_us, their_us = [], []
            for _ in range(3):      # interleaved rounds: kernels, torch, kernels, ...
                mine_us.append(timed(mine, reps=20))
                if theirs is not None:
                    their_us.append(timed(theirs, reps=5, warm=2))
            m = statistics.median(mine_us)
            line = (f"  {name:28s} {m:8.1f} us (min {min(mine_us):.1f}, max {max(mine_us):.1f})  {nbytes / 1e6:7.1f} MB  "
                    f"{nbytes / m / 1e6:5.2f} TB/s = {nbytes / m / 1e6 / COPY_TBS:4.0%} of the copy rate")
            if their_us:
                t = statistics.median(their_us)
                line += f";  torch {t:9.1f} us (min {min(their_us):.1f}, max {max(their_us):.1f}), {t / m:5.1f} x"
            print(line, flush=True)
        del a, b, ga, gb, ar, br
        torch.cuda.empty_cache()


def one_band():
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import point_loss_ref as R
    dev = torch.device("cuda", 0)
    out = {}
    for which in ("fwd", "bwd"):
        for mode in ("kl", "entropy", "focal"):
            mine, n = R.large_errors(which, mode, dev)
            out[f"{which}.{mode}"] = {"N": n, "kernels": mine, "ratio": {k: (mine[k] / n[k] if n[k] else float("inf")) for k in n}}
            print(which, mode, json.dumps(out[f"{which}.{mode}"]), flush=True)
    print(json.dumps({k: v["N"] for k, v in out.items()}, indent=1), flush=True)


# ---- the trainer band -------------------------------------------------------------------------------------------------------------------------

def band_run(kind, out_dir):
    """kind: "ref" (torch.optim.SGD on dense gradients; ICL_CONV_SPLIT from the environment), "eager" or "captured" (the fused trainer)."""
    import torch
    vol, lab = batch()
    model, tr = build_trainer(dict(OPTIONS), factored=(kind != "ref"), max_iterations=10)
    if kind == "ref":
        opt = torch.optim.SGD(model.parameters(), foreach=False, **SGD)

        class Plain:
            param_groups = opt.param_groups

            def zero_grad(self, set_to_none=True):
                opt.zero_grad(set_to_none=set_to_none)

            def step(self):
                opt.step()

            def abandon_step(self):
                pass
        tr.optimizer = Plain()
    p = dict(model.named_parameters())
    losses, cons, ents, snaps = [], [], [], {}
    if kind == "captured":
        tr.capture(vol, lab, warmup=2)
        losses += [None, None]
        cons += [None, None]
        ents += [None, None]
    while len(losses) < 4:
        r = tr.step(vol, lab)
        losses.append(float(r["loss"]))
        cons.append(float(r["con"]))
        ents.append(float(r["ent"]))
        if len(losses) >= 3:
            snaps[len(losses)] = {k: p[k].detach().cpu().clone() for k in BAND_TENSORS}
    torch.save({"losses": losses, "con": cons, "ent": ents, "snaps": snaps},
               os.path.join(out_dir, f"band_{kind}_{os.environ.get('ICL_CONV_SPLIT', '1')}.pt"))
    print(kind, os.environ.get("ICL_CONV_SPLIT", "1"), "losses", losses, "con", cons, "ent", ents, flush=True)


def band_compare(out_dir):
    import torch

    def rms(a, b):
        a, b = a.double(), b.double()
        return float(((a - b) ** 2).mean().sqrt() / (b ** 2).mean().sqrt())
    r1, r0, ea, ca = (torch.load(os.path.join(out_dir, f)) for f in ("band_ref_1.pt", "band_ref_0.pt", "band_eager_1.pt", "band_captured_1.pt"))
    out = {"N": {}, "captured_vs_eager": {}}
    for t in (3, 4):
        for k in BAND_TENSORS:
            out["N"][f"{k}@{t}"] = rms(r0["snaps"][t][k], r1["snaps"][t][k])
            out["captured_vs_eager"][f"{k}@{t}"] = rms(ca["snaps"][t][k], ea["snaps"][t][k])
    out["N"]["losses"] = [abs(a - b) / abs(b) for a, b in zip(r0["losses"], r1["losses"])]
    out["captured_vs_eager"]["losses"] = [None if a is None else abs(a - b) / abs(b) for a, b in zip(ca["losses"], ea["losses"])]
    out["eager"] = {k: ea[k] for k in ("losses", "con", "ent")}
    out["captured"] = {k: ca[k] for k in ("losses", "con", "ent")}
    print(json.dumps(out, indent=1), flush=True)


def child(args, limit, env=None):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__)] + args
    print("+", " ".join(cmd[4:]), flush=True)
    rc = subprocess.run(cmd, env={**os.environ, **(env or {})}).returncode
    if rc != 0:
        sys.exit(f"point_loss_probe: {' '.join(args)} ended with {rc}; nothing further is started")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--band", action="store_true")
    ap.add_argument("--trainer-band", metavar="DIR")
    ap.add_argument("--one", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        kind, _, arg = a.one.partition(":")
        {"kernels": one_kernels, "band": one_band, "band_ref": lambda: band_run("ref", arg), "band_eager": lambda: band_run("eager", arg),
         "band_captured": lambda: band_run("captured", arg), "band_compare": lambda: band_compare(arg)}[kind]()
    elif a.band:
        child(["--one", "band"], 240)
    elif a.trainer_band:
        os.makedirs(a.trainer_band, exist_ok=True)
        child(["--one", f"band_ref:{a.trainer_band}"], 300, {"ICL_CONV_SPLIT": "1"})
        child(["--one", f"band_ref:{a.trainer_band}"], 300, {"ICL_CONV_SPLIT": "0"})
        child(["--one", f"band_eager:{a.trainer_band}"], 300, {"ICL_CONV_SPLIT": "1"})
        child(["--one", f"band_captured:{a.trainer_band}"], 300, {"ICL_CONV_SPLIT": "1"})
        child(["--one", f"band_compare:{a.trainer_band}"], 120)
    else:
        child(["--one", "kernels"], 300)


if __name__ == "__main__":
    main()
