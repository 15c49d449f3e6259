"""The AdamW kernels (csrc/kernels/adamw.h), their launchers and icl_amd.optim.FusedAdamW on the MI355X: every entry of
tests/adamw_ref.py's table exactly as test_adamw_emu.py runs it on the emulation, the many-workgroup factored case, and
ICLTrainer(optimizer="adamw") on the 96^3 unet_3D_icl (nc = 2) — eager against the same trainer with torch.optim.AdamW on dense
gradients, captured against eager, and a state dict taken after capture() against the next replay.

Band of the trainer checks: N = the rms difference (conftest.rms_err: rms(a - b) / rms(b)) between two runs of the torch.optim.AdamW loop
that differ only in ICL_CONV_SPLIT (1 and 0) — both legitimate fp32-grade gradient evaluations — measured per tensor and per loss with
`python tools/adamw_probe.py --band DIR` on an MI355X, each run in its own process (profiles/adamw.md §4).  The tests assert <= 2 N.
rms, not the max-norm: Adam's g / (|g| + eps) turns rounding noise on near-zero gradient elements into lr-sized differences on isolated
elements."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import adamw_ref as ref  # noqa: E402
from conftest import rms_err  # noqa: E402

from icl_amd.utils.hashfill import fill_like_reference_init, synthetic_labels, synthetic_volume  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from icl_amd import _lib
    assert _lib.lib_path().endswith("libicl_hip.so"), "GPU tests must run on the HIP library"
    return torch.device("cuda", 0)


@pytest.mark.parametrize("name", list(ref.CHECKS) + list(ref.GPU_CHECKS))
def test_adamw(dev, name):
    {**ref.CHECKS, **ref.GPU_CHECKS}[name](dev)


# ---- ICLTrainer(optimizer="adamw") --------------------------------------------------------------------------------------------------------

BASE_LR, WEIGHT_DECAY, MAX_ITER = 1e-3, 1e-2, 10
TENSORS = ("final.weight", "sspa.class_decoders.2.mlp2.fc1.weight", "sspa.class_decoders.2.norm2.bias")
# N, measured with `python tools/adamw_probe.py --band DIR` (MI355X, profiles/adamw.md §4): rms difference after four steps between the
# torch.optim.AdamW loop under ICL_CONV_SPLIT=1 and under ICL_CONV_SPLIT=0
N_TENSOR = {"final.weight": 5.31e-7, "sspa.class_decoders.2.mlp2.fc1.weight": 1.247e-2, "sspa.class_decoders.2.norm2.bias": 3.34e-4}
# relative difference of the loss of steps 1 .. 4 between the same two runs (step 1: the two forward passes gave the same fp32 loss, and
# the code under test shares its forward pass with the reference, so 0 holds)
N_LOSS = (0.0, 6.58e-5, 1.32e-3, 4.06e-3)


def rms_dev(a, b):
    """conftest.rms_err's formula in fp64 on the device (the 13,824^2 matrix: 191 M elements)."""
    a, b = a.double(), b.double()
    return float(torch.sqrt(((a - b) ** 2).mean() / torch.clamp((b ** 2).mean(), min=1e-60)))


def tensor_err(a, b):
    return rms_dev(a, b) if a.numel() > (1 << 24) else rms_err(a.cpu().numpy(), b.cpu().numpy())


def _trainer(dev, factored=True):
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
    tr = ICLTrainer(model, ICLConfig(num_classes=2, labeled_bs=1, max_iterations=MAX_ITER, optimizer="adamw", base_lr=BASE_LR,
                                     weight_decay=WEIGHT_DECAY, factored_mlp2_grads=factored))
    return model, tr


def _snapshot(model):
    p = dict(model.named_parameters())
    return {k: p[k].detach().clone() for k in TENSORS}


def _steps_of(tr):
    return sorted({float(s["step"]) for s in tr.optimizer.state.values() if "step" in s})


@pytest.fixture(scope="module")
def runs(dev):
    """Every trainer run of this file, once: "eager" (FusedAdamW, four steps), "reference" (torch.optim.AdamW(foreach=False) on dense
    gradients, four steps), "captured" (capture(warmup=2) + two replays) and "restored" (a fresh eager FusedAdamW trainer loaded with the
    captured trainer's model and optimiser state right after capture(), one step)."""
    from icl_amd.optim import FusedAdamW
    vol = synthetic_volume((2, 1, 96, 96, 96), 1337).to(dev)
    lab = synthetic_labels((1, 96, 96, 96), 4242, 2).to(dev)
    out = {}

    model, tr = _trainer(dev)
    assert type(tr.optimizer) is FusedAdamW
    losses, snaps = [], []
    for _ in range(4):
        losses.append(float(tr.step(vol, lab)["loss"]))
        snaps.append(_snapshot(model) if len(losses) >= 3 else None)
    assert all(getattr(p, "_icl_factors", None) is None for p in model.parameters())
    out["eager"] = dict(losses=losses, after3=snaps[2], after4=snaps[3], steps=_steps_of(tr), iter_num=tr.iter_num,
                        n_state=len(tr.optimizer.state))
    del tr, model
    torch.cuda.empty_cache()

    model, tr = _trainer(dev, factored=False)
    tr.optimizer = torch.optim.AdamW(model.parameters(), lr=BASE_LR, betas=(0.9, 0.999), eps=1e-8, weight_decay=WEIGHT_DECAY, foreach=False)
    losses = [float(tr.step(vol, lab)["loss"]) for _ in range(4)]
    out["reference"] = dict(losses=losses, after4=_snapshot(model))
    del tr, model
    torch.cuda.empty_cache()

    model, tr = _trainer(dev)
    tr.capture(vol, lab, warmup=2)
    model_state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    opt_state = copy.deepcopy(tr.optimizer.state_dict())
    after_capture = dict(steps=_steps_of(tr), iter_num=tr.iter_num)
    losses, snaps, hypers = [], [], []
    for _ in range(2):
        losses.append(float(tr.step(vol, lab)["loss"].clone()))
        snaps.append(_snapshot(model))
        hypers.append(tr.hyper_dev.cpu().numpy().copy())
    out["captured"] = dict(losses=losses, after3=snaps[0], after4=snaps[1], steps=_steps_of(tr), iter_num=tr.iter_num, hyper=hypers,
                           after_capture=after_capture, n_state=len(tr.optimizer.state))
    del tr, model
    torch.cuda.empty_cache()

    model, tr = _trainer(dev)
    model.load_state_dict(model_state)
    tr.optimizer.load_state_dict(opt_state)
    tr.iter_num = after_capture["iter_num"]
    loss = float(tr.step(vol, lab)["loss"])
    out["restored"] = dict(losses=[loss], after3=_snapshot(model), steps=_steps_of(tr))
    del tr, model, model_state, opt_state
    torch.cuda.empty_cache()
    return out


def _within(name, got, want, n):
    e = tensor_err(got, want)
    print(f"{name}: rms_err {e:.3e}  N {n:.3e}  ratio {e / n:.2f} (asserted <= 2)")
    return e <= 2.0 * n


def test_trainer_eager_matches_torch_adamw_on_dense_gradients(runs):
    """Four steps of ICLTrainer(optimizer="adamw") — factored mlp2 gradients, multi-tensor launches — against the same trainer with
    factored_mlp2_grads=False and torch.optim.AdamW(foreach=False): final.weight, one 13,824^2 mlp2.fc1.weight, one LayerNorm bias and the
    four losses inside 2 N."""
    a, r = runs["eager"], runs["reference"]
    assert a["iter_num"] == 4 and a["steps"] == [4.0]
    ok = [_within(k, a["after4"][k], r["after4"][k], N_TENSOR[k]) for k in TENSORS]
    for i, (x, y, n) in enumerate(zip(a["losses"], r["losses"], N_LOSS)):
        e = abs(x - y) / abs(y)
        print(f"loss of step {i + 1}: fused {x:.7f} vs torch {y:.7f}  rel {e:.3e}  N {n:.3e}")
        ok.append(e <= 2.0 * n)
    assert all(ok), ok


def test_trainer_captured_steps_equal_eager_steps(runs):
    """capture(warmup=2) + two replays against four eager steps: iter_num and every parameter's ``step`` are 4 on both sides, hyper_dev
    holds the scalars of the step just replayed, weights and losses inside 2 N."""
    a, c = runs["eager"], runs["captured"]
    assert c["after_capture"] == dict(steps=[2.0], iter_num=2)      # the captured step() did not advance the host's counters
    assert c["iter_num"] == a["iter_num"] == 4 and c["steps"] == a["steps"] == [4.0] and c["n_state"] == a["n_state"]
    for t, got in zip((3, 4), c["hyper"]):
        lr = BASE_LR * (1.0 - (t - 2) / MAX_ITER) ** 0.9      # the poly schedule: computed from the pre-increment iter of the step before
        want = np.array([1.0 - lr * WEIGHT_DECAY, lr / (1.0 - 0.9 ** t), (1.0 - 0.999 ** t) ** 0.5], dtype=np.float32)
        assert got.view(np.int32).tolist() == want.view(np.int32).tolist(), (t, got, want)
    ok = [_within(f"{k} after {t}", c[f"after{t}"][k], a[f"after{t}"][k], N_TENSOR[k]) for t in (3, 4) for k in TENSORS]
    for t, x in zip((3, 4), c["losses"]):
        y, n = a["losses"][t - 1], N_LOSS[t - 1]
        e = abs(x - y) / abs(y)
        print(f"loss of step {t}: replayed {x:.7f} vs eager {y:.7f}  rel {e:.3e}  N {n:.3e}")
        ok.append(e <= 2.0 * n)
    assert all(ok), ok


def test_state_dict_after_capture_resumes_in_an_eager_trainer(runs):
    """optimizer.state_dict() taken after capture() (two warm-up steps) loads into a fresh eager FusedAdamW trainer; its next step matches
    the captured trainer's next replay inside 2 N."""
    c, f = runs["captured"], runs["restored"]
    assert f["steps"] == [3.0]
    ok = [_within(k, f["after3"][k], c["after3"][k], N_TENSOR[k]) for k in TENSORS]
    e = abs(f["losses"][0] - c["losses"][0]) / abs(c["losses"][0])
    print(f"loss of step 3: restored {f['losses'][0]:.7f} vs replayed {c['losses'][0]:.7f}  rel {e:.3e}  N {N_LOSS[2]:.3e}")
    assert all(ok) and e <= 2.0 * N_LOSS[2], (ok, e)
