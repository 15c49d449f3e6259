"""More than 16 classes through the training kernels on the device: the cases of tests/many_classes_ref.py (generic-class losses,
class-tiled prototype attention, the small aligner) and the 17-class unet_3D_icl training step against the reference golden
tests/golden/many_classes.npz (tests/golden/make_golden_many_classes.py), eagerly on both convolution paths and as hipGraph replays."""
import numpy as np
import pytest
import torch

import many_classes_ref as M
from conftest import load_golden, rel_err
from icl_amd.utils.hashfill import fill_like_reference_init, synthetic_labels, synthetic_volume

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from icl_amd import _lib
    assert _lib.lib_path().endswith("libicl_hip.so"), "GPU tests must run on the HIP library"
    return torch.device("cuda", 0)


@pytest.mark.parametrize("nc,S,scale", M.LOSS_CASES)
def test_losses_beyond_16_classes_match_torch(dev, nc, S, scale):
    M.check_losses(nc, S, scale, dev)


def test_all_loss_terms_in_one_launch_beyond_16_classes(dev):
    nc, S = 17, (6, 8, 10)
    multi = M.run_multi(nc, S, dev, single=False)
    again = M.run_multi(nc, S, dev, single=False)
    single = M.run_multi(nc, S, dev, single=True)
    assert multi[0] == again[0] == single[0]
    for a, b, c in zip(multi[1], again[1], single[1]):
        assert torch.equal(a, b) and torch.equal(a, c)
    M.assert_multi_close(multi, M.multi_reference(nc, S), "fused_losses nc=17")


@pytest.mark.parametrize("nc", [2, 3, 16])
def test_forced_generic_path_agrees_with_the_register_path(dev, monkeypatch, nc):
    S = (6, 5, 7)
    monkeypatch.delenv("ICL_LOSS_GENERIC", raising=False)
    reg, reg_multi = M.run_losses(nc, S, 1.0, dev), M.run_multi(nc, S, dev, single=False)
    monkeypatch.setenv("ICL_LOSS_GENERIC", "1")
    gen, gen2 = M.run_losses(nc, S, 1.0, dev), M.run_losses(nc, S, 1.0, dev)
    gen_multi = M.run_multi(nc, S, dev, single=False)
    M.assert_bit_equal(gen, gen2, f"generic nc={nc}")
    M.assert_losses_close(gen, reg, f"generic vs register nc={nc}")
    M.assert_losses_close(gen, M.loss_reference(nc, S, 1.0), f"generic vs torch nc={nc}")
    M.assert_multi_close(gen_multi, reg_multi, f"generic vs register, multi, nc={nc}")
    M.assert_multi_close(gen_multi, M.multi_reference(nc, S), f"generic vs torch, multi, nc={nc}")


def test_257_classes_raise_a_value_error_naming_the_limit(dev):
    from icl_amd import ops
    a = torch.zeros(1, 257, 8, device=dev)
    lab = torch.zeros(1, 8, dtype=torch.int64, device=dev)
    with pytest.raises(ValueError, match="256"):
        ops.cross_entropy_dice_parts(a, lab, 257)
    with pytest.raises(ValueError, match="256"):
        ops.prototype_attention(torch.zeros(1, 2, 257, 8, device=dev), torch.zeros(1, 5, 32, device=dev), 2, 1.0)
    assert ops.MAX_CLASSES == 256


@pytest.mark.parametrize("B,h,nc,d,N", M.ATTN_CASES)
def test_prototype_attention_beyond_16_classes(dev, B, h, nc, d, N):
    M.check_attention(B, h, nc, d, N, dev)


@pytest.mark.parametrize("tag,train", [("tr", True), ("ev", False)])
def test_small_aligner_at_17_classes_matches_reference_golden(dev, tag, train):
    M.check_aligner(dev, load_golden("many_classes.npz"), tag, train)


def _model(dev, nc, **cfg):
    from icl_amd import ops
    from icl_amd.networks.aligner import DropPath
    from icl_amd.networks.layers import Dropout3
    from icl_amd.networks.unet_3D_icl import unet_3D_icl
    from icl_amd.trainer import ICLConfig, ICLTrainer
    ops.StepRNG.tensor = None
    model = unet_3D_icl(n_classes=nc, in_channels=1, device=dev)
    fill_like_reference_init(list(model.named_parameters()))
    for mod in model.modules():      # parity mode, as tests/test_gpu_parity.py
        if isinstance(mod, Dropout3):
            mod.p = 0.0
        if isinstance(mod, DropPath):
            mod.drop_prob = 0.0
    model.train()
    return model, ICLTrainer(model, ICLConfig(num_classes=nc, labeled_bs=1, **cfg))


def _batch(dev, nc):
    return synthetic_volume((2, 1, 96, 96, 96), 1337).to(dev), synthetic_labels((1, 96, 96, 96), 4242, nc).to(dev)


@pytest.mark.parametrize("split", ["1", "0"])
def test_unet3d_icl_17_class_step_matches_reference_golden(dev, monkeypatch, split):
    """One training step of unet_3D_icl at 17 classes, 96^3, batch 1 + 1, on the split-product and on the exact-fp32 convolutions.
    Bands: those tests/test_gpu_parity.py::test_full_icl_step_matches_reference_golden applies to the same quantities of the 16-class
    golden — logits 1e-3, loss terms 1e-4 absolute, grad.final.weight 1e-3 (final.bias with it: the same layer's gradient),
    grad.sspa.guided_Q 5e-3, gradient norms of the encoder weights 1e-2 — and, element-wise on the two encoder gradients, the 2e-2 of
    the deep-gradient comparisons there."""
    monkeypatch.setenv("ICL_CONV_SPLIT", split)
    nc = M.GOLDEN_NC
    g = load_golden("many_classes.npz")
    model, tr = _model(dev, nc)
    vol, lab = _batch(dev, nc)
    outs = model(vol[:1], vol[1:])
    logits = outs[0].detach().reshape(-1).cpu().numpy()
    e = rel_err(logits[M.sample_index(logits.size, M.LOGIT_SAMPLES)], g["step_logits"])
    print(f"split={split} logits rel_err {e:.2e} (band 1e-3)")
    assert e < 1e-3
    loss, parts = tr.compute_loss(outs, lab)
    got = [float(parts[k]) for k in ("dice", "ce", "aux", "pse", "con")] + [float(loss)]
    print(f"split={split} losses {got} vs {list(g['step_losses'])}")
    assert np.allclose(got, g["step_losses"], rtol=0, atol=1e-4), (got, g["step_losses"])
    tr.optimizer.zero_grad(set_to_none=True)
    loss.backward()
    p = dict(model.named_parameters())
    errs = {k: rel_err(p[k].grad.cpu(), g["step_grad." + k]) for k in ("final.weight", "final.bias", "sspa.guided_Q", "conv1.conv1.0.weight")}
    sub = p["center.conv2.0.weight"].grad[::16, ::16].cpu()
    errs["center.conv2.0.weight_sub"] = rel_err(sub, g["step_grad.center.conv2.0.weight_sub"])
    print(f"split={split} gradient rel_err", {k: f"{v:.2e}" for k, v in errs.items()})
    assert errs["final.weight"] < 1e-3 and errs["final.bias"] < 1e-3 and errs["sspa.guided_Q"] < 5e-3, errs
    assert errs["conv1.conv1.0.weight"] < 2e-2 and errs["center.conv2.0.weight_sub"] < 2e-2, errs
    for k, t in (("conv1.conv1.0.weight", p["conv1.conv1.0.weight"].grad), ("center.conv2.0.weight_sub", sub)):
        rn = float(np.linalg.norm(g["step_grad." + k].astype(np.float64)))
        assert abs(float(t.double().norm()) - rn) <= 1e-2 * rn, k


def test_unet3d_icl_17_class_graph_replay_equals_eager_steps(dev):
    """ICLTrainer.capture at 17 classes: 2 warm-up + 2 replayed steps against 4 eager steps, the losses of steps 3 and 4 within the
    band of tests/test_gpu_parity.py::test_graph_replay_equals_eager_steps (rtol 1e-4); the first eager step is the golden's."""
    nc = M.GOLDEN_NC
    g = load_golden("many_classes.npz")
    vol, lab = _batch(dev, nc)
    runs = []
    for graphed in (False, True):
        model, tr = _model(dev, nc, max_iterations=10)
        if graphed:
            tr.capture(vol, lab, warmup=2)
            losses = [float(tr.step(vol, lab)["loss"].clone()) for _ in range(2)]
        else:
            parts = tr.step(vol, lab)
            first = [float(parts[k]) for k in ("dice", "ce", "aux", "pse", "con", "loss")]
            assert np.allclose(first, g["step_losses"], rtol=0, atol=1e-4), (first, g["step_losses"])
            losses = [float(tr.step(vol, lab)["loss"].clone()) for _ in range(3)][1:]
        assert tr.iter_num == 4
        runs.append(losses)
        del tr, model
        torch.cuda.empty_cache()
    print("eager", runs[0], "replayed", runs[1])
    assert np.allclose(runs[0], runs[1], rtol=1e-4), runs


@pytest.mark.parametrize("B,h,nc,d,N", M.ATTN_SMALL_CASES)
def test_forced_class_tiles_agree_with_the_single_tile_kernels(dev, monkeypatch, B, h, nc, d, N):
    """ICL_ATTN_TILED=1 sends any class count through the class-tiled logits and dK / dV kernels: within the bands of torch and of the
    single-tile kernels' results on the same inputs."""
    monkeypatch.delenv("ICL_ATTN_TILED", raising=False)
    plain = M.run_attention(B, h, nc, d, N, dev)
    monkeypatch.setenv("ICL_ATTN_TILED", "1")
    M.check_attention(B, h, nc, d, N, dev)
    M.check_attention(B, h, nc, d, N, dev, against=plain)
