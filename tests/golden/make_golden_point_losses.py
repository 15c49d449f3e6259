"""Data-only generator of tests/golden/point_losses.npz: the reference's own softmax_kl_loss, compute_kl_loss, FocalLoss,
entropy_minmization and entropy_map on the small inputs of tests/point_loss_ref.py.

    python tests/golden/make_golden_point_losses.py [--out tests/golden]

Like make_golden.py it imports the reference implementation from /root/reference/code and runs it on the CPU, here in fp64.  Per case of
``point_loss_ref.golden_cases()``: the fp32 inputs (``NAME.in0`` ..), the value or map (``NAME.out``) and the gradient of every input that
takes one (``NAME.grad0`` ..) under the case's upstream gradient.  entropy_loss and entropy_loss_map call .cuda() in the reference and
cannot run here; they are entropy_minmization / entropy_map divided by log C.
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as G  # noqa: E402
import point_loss_ref as P  # noqa: E402


def reference_functions(L):
    """name of a golden case -> the reference's function for it."""
    fns = {f"kl{nc}": L.softmax_kl_loss for nc in (2, 3, 16)}
    fns["kl_extreme"] = L.softmax_kl_loss
    fns["compute_kl"] = lambda *x: L.compute_kl_loss(list(x[:3]), list(x[3:]))
    fns["entropy_min3"] = L.entropy_minmization
    fns["entropy_map3"] = L.entropy_map
    fns["focal2_g2_mean"] = lambda v, t: L.FocalLoss(2, P.FOCAL_ALPHA[2], True)(v, t)
    fns["focal3_g1.5_sum"] = lambda v, t: L.FocalLoss(1.5, P.FOCAL_ALPHA[3], False)(v, t)
    fns["focal3_g0_mean"] = lambda v, t: L.FocalLoss(0, P.FOCAL_ALPHA[3], True)(v, t)
    fns["focal_rows"] = lambda v, t: L.FocalLoss(2, None, True)(v, t)
    return fns


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args()
    L = G.import_reference()["losses"]
    fns = reference_functions(L)
    cases = P.golden_cases()
    assert set(fns) == set(cases), set(fns) ^ set(cases)
    d = {}
    for name, (_, tensors, needs, up) in cases.items():
        outs, grads = P.evaluate(fns[name], tensors, needs, "cpu", dtype=torch.float64, upstream=up)
        for i, t in enumerate(tensors):
            d[f"{name}.in{i}"] = t.numpy()
        d[f"{name}.out"] = outs[0].numpy()
        for i, g in enumerate(grads):
            if g is not None:
                d[f"{name}.grad{i}"] = g.numpy()
        print(name, "value", float(outs[0].reshape(-1)[0]))
    path = os.path.join(a.out, "point_losses.npz")
    np.savez_compressed(path, **d)
    print("point_losses.npz", os.path.getsize(path) / 1e3, "KB")
