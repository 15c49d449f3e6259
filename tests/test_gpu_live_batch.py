"""Live batch on the MI355X (DESIGN.md §4.4 "Live batch"): the backward of the upper decoder on the live samples of a gradient whose tail is exactly
zero.  The parent's behaviour — ICL_LIVE_BATCH=0, the same launches as before the mark existed — is the reference of every check.

Operator level: batch 3 with k = 1 and k = 2 live samples (one live or one dead sample hides prefix and stride mistakes), the shapes
the smallest at which the launchers still pick the templates of the 96^3 / 48^3 layers of the step (asserted through
icl_last_kernel_name).  Live samples of every input gradient bit for bit, tails zero; weight / bias gradients bit for bit as well: the
weight-gradient launches keep the slab plan of the full batch and skip the workgroups that own no live tile.  Model
level: one trainer step of a small unet_3D_icl."""
import pytest
import torch

import live_batch_checks as C
from icl_amd.utils.hashfill import fill_like_reference_init, synthetic_labels, synthetic_volume

pytestmark = pytest.mark.gpu

# Every weight / bias gradient keeps the slab plan of the full batch: no band, bitwise equality (a first form of this change planned the
# weight gradients for the live batch alone and re-associated them by up to 4.75e-7 of the max-norm: profiles/live_batch.md).
OP_BAND = 0.0


@pytest.fixture(scope="module")
def dev():
    from icl_amd import _lib
    assert _lib.lib_path().endswith("libicl_hip.so"), "GPU tests must run on the HIP library"
    return torch.device("cuda", 0)


def _report(tag, rep):
    print(f"live-batch deviation {tag}: " + ", ".join(f"{n} {d:.3e}" for n, d in rep))


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("cin,cout,d,h,w,wgrad,dgrad,live", [
    # 16 -> 16: 13,824 voxels, the split-product kernels' threshold; the loader-wave kernel of the 96^3 layers
    (16, 16, 18, 24, 32, "conv3d_wgrad_zs_kernel<1, 10>", "conv3d_bf16x3_fwd_ws_kernel<1>", True),
    # 48 -> 16: exchanged-roles weight gradient, 16 -> 48 input gradient (three cout blocks; rows of 24 voxels: the flat tile)
    (48, 16, 24, 24, 24, "conv3d_wgrad_zs_kernel<3, 8>", "conv3d_bf16x3_fwd_kernel<3, 8, 60, flat24>", True),
    # rows of 24 voxels, two chunks: the input gradient's split follows the batch size
    (32, 32, 24, 24, 24, "conv3d_wgrad_zs_kernel<2, 8>", "conv3d_bf16x3_fwd_kernel<2, 8, 60, flat24>", None),
    # ... and rows the 48^3 level's kernel takes
    (32, 32, 18, 24, 32, "conv3d_wgrad_zs_kernel<2, 8>", "conv3d_bf16x3_fwd_kernel<2, 8, 60>", True),
])
def test_conv_norm_backward_on_the_live_samples(dev, monkeypatch, k, cin, cout, d, h, w, wgrad, dgrad, live):
    """_Conv3d + _NormAct.  live None: the launcher decides (icl_conv3d_fwd_live_ok: at 24^3 the split count of a 32-channel input
    gradient follows the batch size, a live batch of one would re-associate the live samples — it runs the full batch there)."""
    from icl_amd import _lib
    res = C.run_pair(monkeypatch, C.conv_norm_case(dev, 3, cin, cout, d, h, w), k)
    rep = []
    C.compare(res, k, batched={"x"}, band="later", report=rep)
    _report(f"conv {cin}->{cout} {d}x{h}x{w} k={k}", rep)
    C.check_band(rep, OP_BAND)
    assert res["kernel"] == wgrad, res["kernel"]
    marked = ((3, cin, d, h, w), k) in res["marks"] if cin != cout else res["marks"].count(((3, cin, d, h, w), k)) == 3
    expect = bool(_lib.lib().icl_conv3d_fwd_live_ok(3, k, cout, cin, d, h, w)) if live is None else live
    assert marked == expect, res["marks"]
    launched, planned = res["wgrad_grid"]
    if expect:
        # the live path really ran: the input gradient on the workload's template, the weight gradient on a prefix of its plan's grid
        assert res["live_fwd_kernel"] == dgrad, res["live_fwd_kernel"]
        assert 0 < launched < planned and launched <= -(-planned * k // 3) + 1, (launched, planned)
    else:
        assert launched == planned > 0, (launched, planned)


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("d,h,w", [(24, 24, 24), (18, 24, 32)])
def test_upcat_decoder_block_on_the_live_samples(dev, monkeypatch, k, d, h, w):
    """up_concat2's shape class: cat([skip 32, up2x(deep 64)]) -> 96 -> 32 -> 32 with InstanceNorm + ReLU (_UpCat and its up-sampling
    backward, _Conv3d, _NormAct)."""
    res = C.run_pair(monkeypatch, C.upcat_case(dev, 3, 32, 64, 32, d, h, w), k)
    rep = []
    C.compare(res, k, batched={"skip", "deep"}, band="later", report=rep)
    _report(f"upcat 96->32->32 {d}x{h}x{w} k={k}", rep)
    C.check_band(rep, OP_BAND)
    assert res["kernel"] == "conv3d_wgrad_zs_kernel<2, 8>", res["kernel"]
    if w != 24:
        assert ((3, 96, d, h, w), k) in res["marks"] and ((3, 64, d // 2, h // 2, w // 2), k) in res["marks"], res["marks"]
        assert res["live_fwd_kernel"] == "conv3d_bf16x3_fwd_kernel<3, 8, 60>", res["live_fwd_kernel"]      # 32 -> 96 input gradient
        launched, planned = res["wgrad_grid"]
        assert 0 < launched < planned, (launched, planned)


@pytest.mark.parametrize("k", [1, 2])
def test_deferred_norm_backward_on_the_live_samples(dev, monkeypatch, k):
    """_NormActLazy at a volume of several chunks per row (partial + apply kernels)."""
    res = C.run_pair(monkeypatch, C.lazy_norm_case(dev, 3, 16, 18, 24, 32), k)
    C.compare(res, k, batched={"y"})
    assert res["marks"] == [((3, 16, 18, 24, 32), k)] * 2


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("p,lazy,w", [(0.3, True, 64), (0.3, False, 64), (0.0, True, 64), (0.0, False, 64), (0.3, True, 32)])
def test_final_layer_on_the_live_samples(dev, monkeypatch, k, p, lazy, w):
    """The fused `final` layer, 16 -> 2 on 32 x 32 x 64 (n_live * S >= 65,536 from k = 1 on) and on 32^3 (one live sample alone is below
    the big-volume kernels' threshold; it runs the full batch's kernel): _DropoutConv1x1Lazy, _DropoutConv1x1 and the <= 16-channel
    _Conv3d; the dropout mask of the live samples is the full batch's (bitwise equal input gradients say so)."""
    res = C.run_pair(monkeypatch, C.final_case(dev, 3, 16, 2, 32, 32, w, p, lazy), k)
    rep = []
    C.compare(res, k, batched={"t"}, band="later", report=rep)
    _report(f"final p={p} lazy={lazy} 32x32x{w} k={k}", rep)
    C.check_band(rep, OP_BAND)
    assert ((3, 16, 32, 32, w), k) in res["marks"], res["marks"]


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("lazy", [False, True])
def test_skip_and_pool_skips_the_dead_addend(dev, monkeypatch, k, lazy):
    """maxpool2_bwd_add_x2_kernel with skip_live at 16^3: the skip gradient is the marked channel-slice view of the concat gradient (as
    _UpCat.backward produces it), the pooling gradient a full batch: x's gradient equals the full run's in every sample, bit for bit."""
    res = C.run_pair(monkeypatch, C.skip_pool_case(dev, 3, 16, 32, 16, 16, 16, lazy), k)
    C.compare(res, k, batched={"deep"}, full={"x"})
    assert ((3, 16, 16, 16, 16), k) in res["marks"] and ((3, 32, 8, 8, 8), k) in res["marks"], res["marks"]


# ---- model level -------------------------------------------------------------------------------------------------------------------

def _small_model(dev):
    from icl_amd.networks.unet_3D_icl import unet_3D_icl
    torch.manual_seed(1337)
    model = unet_3D_icl(n_classes=2, in_channels=1, device=dev, icl_in_resolutions=(2, 4, 8))
    fill_like_reference_init(list(model.named_parameters()))
    model.train()
    return model


def _trainer(model, **kw):
    from icl_amd.trainer import ICLConfig, ICLTrainer
    return ICLTrainer(model, ICLConfig(num_classes=2, labeled_bs=1, max_iterations=10, patch_size=(32, 32, 32), **kw))


def _step_grads(dev, monkeypatch, on, differentiate_unlabeled=False):
    """Parameter gradients of the SECOND forward + backward of a fresh small model (the first packs and splits the weights: from the
    second on the convolutions hand the statistics over and the LazyAct path runs); no update between the two."""
    from icl_amd import ops
    monkeypatch.setenv("ICL_LIVE_BATCH", on)
    monkeypatch.setenv("ICL_LAZY_NORM_MIN", str(16 ** 3))
    ops.StepRNG.tensor = None
    vol = synthetic_volume((2, 1, 32, 32, 32), 1337).to(dev)
    lab = synthetic_labels((1, 32, 32, 32), 4242, 2).to(dev)
    model = _small_model(dev)
    tr = _trainer(model, factored_mlp2_grads=False, update_in_backward=False)
    if differentiate_unlabeled:
        base = tr.compute_loss

        def loss_with_unlabeled_logits(outputs, label):
            loss, parts = base(outputs, label)
            return loss + (outputs[1] * outputs[1]).mean(), parts
        tr.compute_loss = loss_with_unlabeled_logits
    spy = C.MarkSpy(monkeypatch)
    for it in range(2):
        torch.manual_seed(7)                   # the dropout seeds of an eager step come from torch's generator
        spy.marks.clear()
        tr._forward_backward(vol, lab)
        tr.optimizer.abandon_step()
    torch.cuda.synchronize(dev)
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    return grads, list(spy.marks)


def test_trainer_step_gradients_equal_the_full_batch_step(dev, monkeypatch):
    """Every parameter gradient of one step, mark on against mark off; the unlabeled sample still trains the aligners and the encoder
    (its gradient reaches them through the aligners' maps of center / up4 / up3)."""
    g0, m0 = _step_grads(dev, monkeypatch, "0")
    g1, m1 = _step_grads(dev, monkeypatch, "1")
    assert not m0 and m1, (m0, m1)
    assert ((2, 2, 32, 32, 32), 1) in m1 and ((2, 16, 32, 32, 32), 1) in m1 and ((2, 48, 32, 32, 32), 1) in m1, m1      # final .. up_concat1
    assert g0.keys() == g1.keys()
    rep = [(n, C.max_norm_dev(g1[n], g0[n])) for n in g0]
    worst = max(rep, key=lambda r: r[1])
    print(f"live-batch deviation, model level: worst {worst[0]} {worst[1]:.3e}; "
          + ", ".join(f"{n} {d:.2e}" for n, d in sorted(rep, key=lambda r: -r[1])[:8]))
    # (conv biases in front of an InstanceNorm: exact zeros in both runs)
    bad = [n for n in g0 if not torch.equal(g0[n], g1[n])]
    assert not bad, bad[:8]
    for head in ("sspa", "uscl", "conv1", "conv2", "conv3", "conv4", "center"):
        live = [n for n in g1 if n.startswith(head + ".") and n.endswith("weight") and float(g1[n].abs().max()) > 0]
        assert live, head


def test_a_loss_on_the_unlabeled_logits_keeps_the_full_batch(dev, monkeypatch):
    """outputs[1] differentiated: autograd hands _SplitBatch both halves, no mark is created, on and off are the same launches."""
    g0, m0 = _step_grads(dev, monkeypatch, "0", differentiate_unlabeled=True)
    g1, m1 = _step_grads(dev, monkeypatch, "1", differentiate_unlabeled=True)
    assert [m for m in m1 if m[0][1:] == (2, 32, 32, 32)] == [] and not m0, m1       # none from the logits' split
    assert g0.keys() == g1.keys() and all(torch.equal(g0[n], g1[n]) for n in g0)


def test_capture_and_two_replays_equal_eager_steps(dev, monkeypatch):
    """The fill nodes of the zero tails and the live launches are captured like everything else: 2 warm-up + 2 replayed steps == 4 eager
    steps (the band of tests/test_gpu_parity.py::test_graph_replay_equals_eager_steps), dropout off so that both draw no masks."""
    from icl_amd import ops
    from icl_amd.networks.aligner import DropPath
    from icl_amd.networks.layers import Dropout3
    from conftest import rel_err
    monkeypatch.setenv("ICL_LIVE_BATCH", "1")
    monkeypatch.setenv("ICL_LAZY_NORM_MIN", str(16 ** 3))
    vol = synthetic_volume((2, 1, 32, 32, 32), 1337).to(dev)
    lab = synthetic_labels((1, 32, 32, 32), 4242, 2).to(dev)
    finals = []
    for graphed in (False, True):
        ops.StepRNG.tensor = None
        model = _small_model(dev)
        for mod in model.modules():
            if isinstance(mod, Dropout3):
                mod.p = 0.0
            if isinstance(mod, DropPath):
                mod.drop_prob = 0.0
        tr = _trainer(model)
        if graphed:
            tr.capture(vol, lab, warmup=2)
            losses = [tr.step(vol, lab)["loss"].clone() for _ in range(2)]
        else:
            losses = [tr.step(vol, lab)["loss"].clone() for _ in range(4)][2:]
        finals.append((model.final.weight.detach().clone(), model.up_concat1.conv.conv1[0].weight.detach().clone(),
                       model.conv1.conv1[0].weight.detach().clone(), [float(v) for v in losses]))
        del tr, model
        torch.cuda.empty_cache()
    ops.StepRNG.tensor = None
    (f0, u0, c0, l0), (f1, u1, c1, l1) = finals
    assert rel_err(f1.cpu(), f0.cpu()) < 1e-5 and rel_err(u1.cpu(), u0.cpu()) < 1e-5 and rel_err(c1.cpu(), c0.cpu()) < 1e-5
    assert all(abs(a - b) <= 1e-4 * abs(a) for a, b in zip(l0, l1)), (l0, l1)
