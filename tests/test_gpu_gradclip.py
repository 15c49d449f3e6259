"""Gradient clipping by the global norm on the MI355X: every entry of tests/gradclip_ref.py's table exactly as test_gradclip_emu.py runs
it on the emulation, the many-workgroup factored cases (8 and 160 rows), and ICLConfig.max_grad_norm in ICLTrainer on the 96^3
unet_3D_icl (nc = 2): (a) a clip that never binds (max_grad_norm = 1e30) leaves three steps of both optimisers bit-identical to the
unclipped trainer, (b) AdamW with a binding clip, captured against eager.

Band of (b): N = the rms difference (conftest.rms_err: rms(a - b) / rms(b)) after four steps between two runs of the torch loop —
torch.optim.AdamW + torch.nn.utils.clip_grad_norm_(MAX_NORM) on dense gradients (factored_mlp2_grads=False) — that differ only in
ICL_CONV_SPLIT (1 and 0): both legitimate fp32-grade evaluations of the same clipped step.  Measured per tensor and per loss with
`python tools/gradclip_probe.py --band DIR --max-norm 0.5` on an MI355X, each run in its own process (profiles/gradclip.md §3).  The tests
assert <= 2 N, the factor the project gives two fp32-grade evaluations (test_gpu_adamw.py)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gradclip_ref as ref  # noqa: E402
from test_gpu_adamw import BASE_LR, MAX_ITER, TENSORS, WEIGHT_DECAY, tensor_err  # noqa: E402

from icl_amd.utils.hashfill import fill_like_reference_init, synthetic_labels, synthetic_volume  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from icl_amd import _lib
    assert _lib.lib_path().endswith("libicl_hip.so"), "GPU tests must run on the HIP library"
    return torch.device("cuda", 0)


@pytest.mark.parametrize("name", list(ref.CHECKS) + list(ref.GPU_CHECKS))
def test_gradclip(dev, name):
    {**ref.CHECKS, **ref.GPU_CHECKS}[name](dev)


# ---- ICLConfig.max_grad_norm ------------------------------------------------------------------------------------------------------------------

# The binding clip of (b): the unclipped total_norm of the first four AdamW steps of this setup is 15.57, 9.49, 3.19, 2.18
# (`python tools/gradclip_probe.py --norms`, profiles/gradclip.md §3); 0.5 is below a quarter of each.
MAX_NORM = 0.5
# N, measured with `python tools/gradclip_probe.py --band DIR --max-norm 0.5` (MI355X, profiles/gradclip.md §3): rms difference after four
# steps between the torch loop (torch.optim.AdamW + torch's clip, dense gradients) under ICL_CONV_SPLIT=1 and under ICL_CONV_SPLIT=0
N_TENSOR = {"final.weight": 1.882e-5, "sspa.class_decoders.2.mlp2.fc1.weight": 1.3317e-2, "sspa.class_decoders.2.norm2.bias": 1.5124e-3}
# relative difference of the loss of steps 1 .. 4 between the same two runs (step 1: the two forward passes gave the same fp32 loss, and
# captured and eager share their forward kernels, so 0 holds)
N_LOSS = (0.0, 4.099e-5, 1.0437e-3, 2.1715e-3)


def _trainer(dev, optimizer, max_grad_norm, **kw):
    from icl_amd import ops
    from icl_amd.networks.aligner import DropPath
    from icl_amd.networks.layers import Dropout3
    from icl_amd.networks.unet_3D_icl import unet_3D_icl
    from icl_amd.trainer import ICLConfig, ICLTrainer
    ops.StepRNG.tensor = None
    model = unet_3D_icl(n_classes=2, in_channels=1, device=dev)
    fill_like_reference_init(list(model.named_parameters()))
    for mod in model.modules():
        if isinstance(mod, Dropout3):
            mod.p = 0.0
        if isinstance(mod, DropPath):
            mod.drop_prob = 0.0
    model.train()
    opt = dict(optimizer="adamw", base_lr=BASE_LR, weight_decay=WEIGHT_DECAY) if optimizer == "adamw" else dict(optimizer="sgd")
    tr = ICLTrainer(model, ICLConfig(num_classes=2, labeled_bs=1, max_iterations=MAX_ITER, max_grad_norm=max_grad_norm, **opt, **kw))
    return model, tr


def _snapshot(model):
    p = dict(model.named_parameters())
    return {k: p[k].detach().clone() for k in TENSORS}


@pytest.fixture(scope="module")
def runs(dev):
    """Every trainer run of this file, once.  (a): "adamw" / "adamw,1e30" and "sgd" (update_in_backward=False) / "sgd,1e30", three
    eager steps each.  (b): "eager" (AdamW, max_grad_norm = MAX_NORM, four steps) and "captured" (capture(warmup=2) + two replays)."""
    vol = synthetic_volume((2, 1, 96, 96, 96), 1337).to(dev)
    lab = synthetic_labels((1, 96, 96, 96), 4242, 2).to(dev)
    out = {}
    for name, optimizer, c, kw in (("adamw", "adamw", None, {}), ("adamw,1e30", "adamw", 1e30, {}),
                                   ("sgd", "sgd", None, dict(update_in_backward=False)), ("sgd,1e30", "sgd", 1e30, {})):
        model, tr = _trainer(dev, optimizer, c, **kw)
        losses, norms = [], []
        for _ in range(3):
            r = tr.step(vol, lab)
            losses.append(float(r["loss"]))
            assert ("grad_norm" in r) == (c is not None)
            if c is not None:
                norms.append(float(r["grad_norm"]))
        assert all(getattr(p, "_icl_factors", None) is None for p in model.parameters())
        out[name] = dict(losses=losses, norms=norms, after3=_snapshot(model))
        del tr, model
        torch.cuda.empty_cache()

    model, tr = _trainer(dev, "adamw", MAX_NORM)
    losses, snaps, clips = [], [], []
    for _ in range(4):
        losses.append(float(tr.step(vol, lab)["loss"]))
        snaps.append(_snapshot(model) if len(losses) >= 3 else None)
        clips.append(tr.optimizer.clip_dev.cpu().numpy().copy())
    out["eager"] = dict(losses=losses, after3=snaps[2], after4=snaps[3], clips=clips)
    del tr, model
    torch.cuda.empty_cache()

    model, tr = _trainer(dev, "adamw", MAX_NORM)
    tr.capture(vol, lab, warmup=2)
    losses, snaps, clips, norms = [], [], [], []
    for _ in range(2):
        r = tr.step(vol, lab)
        losses.append(float(r["loss"].clone()))
        norms.append(float(r["grad_norm"]))
        snaps.append(_snapshot(model))
        clips.append(tr.optimizer.clip_dev.cpu().numpy().copy())
    out["captured"] = dict(losses=losses, after3=snaps[0], after4=snaps[1], clips=clips, norms=norms)
    del tr, model
    torch.cuda.empty_cache()
    return out


@pytest.mark.parametrize("optimizer", ["adamw", "sgd"])
def test_a_clip_that_never_binds_changes_no_bit(runs, optimizer):
    """max_grad_norm = 1e30 (coef == 1: the dense gradients are not touched, the factor rows are copied) against max_grad_norm = None —
    for SGD against update_in_backward=False, which the option implies: three steps, the three tensors and the losses bit for bit;
    "grad_norm" is finite and positive."""
    a, b = runs[optimizer], runs[optimizer + ",1e30"]
    assert a["losses"] == b["losses"], (a["losses"], b["losses"])
    for k in TENSORS:
        assert torch.equal(a["after3"][k].view(torch.int32), b["after3"][k].view(torch.int32)), k
    print(optimizer, "grad_norm of steps 1..3:", b["norms"])
    assert all(np.isfinite(n) and n > 0 for n in b["norms"]) and not a["norms"]


def _within(name, got, want, n):
    e = tensor_err(got, want)
    print(f"{name}: rms_err {e:.3e}  N {n:.3e}  ratio {e / n:.2f} (asserted <= 2)")
    return e <= 2.0 * n


def test_captured_steps_clip_by_their_own_norm(runs):
    """AdamW with a binding clip, capture(warmup=2) + two replays against four eager steps: after each replay clip_dev holds a
    coefficient < 1 that is the fp32 expression of that replay's own norm, the two replays' norms differ, weights and losses inside
    2 N."""
    a, c = runs["eager"], runs["captured"]
    for clip, norm in zip(c["clips"], c["norms"]):
        assert clip[1] < 1.0 and ref.same_f32(clip[1], ref.coef_of(clip[0], MAX_NORM)), clip
        assert ref.same_f32(clip[0], norm)
    assert c["clips"][0][0] != c["clips"][1][0], c["clips"]
    assert all(clip[1] < 1.0 and ref.same_f32(clip[1], ref.coef_of(clip[0], MAX_NORM)) for clip in a["clips"]), a["clips"]
    print("norms: eager", [float(x[0]) for x in a["clips"]], "replayed", c["norms"])
    ok = [_within(f"{k} after {t}", c[f"after{t}"][k], a[f"after{t}"][k], N_TENSOR[k]) for t in (3, 4) for k in TENSORS]
    for t, x in zip((3, 4), c["losses"]):
        y, n = a["losses"][t - 1], N_LOSS[t - 1]
        e = abs(x - y) / abs(y)
        print(f"loss of step {t}: replayed {x:.7f} vs eager {y:.7f}  rel {e:.3e}  N {n:.3e}")
        ok.append(e <= 2.0 * n)
    assert all(ok), ok
