"""Multi-modal volumes on the MI355X (run with -m gpu): the C-channel gather and the channel-wise normalisation through the library
(crop_rotflip_channels_kernel<1 | 4>, channel_norm_partial_kernel<1 | 2>, channel_norm_finish_kernel<1 | 2>, channel_norm_apply_kernel<1 | 4>
in csrc/kernels/datafeed.h), the intensity stage on [B,C,...] batches, the first convolution at 2..4 input channels, the step, the
captured step and SwinUNETR_icl at in_channels = 4, and the validation loops on channel-first cases.  The feed, intensity and
normalisation checks are those of tests/test_multimodal_feed_emu.py, with the same equalities (tests/multimodal_feed_ref.py)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import multimodal_feed_ref as ref  # noqa: E402
from conftest import rel_err  # noqa: E402
from test_multimodal_feed_emu import (check_intensity_one_channel_is_unchanged, check_intensity_per_channel,  # noqa: E402
                                      check_intensity_shared_rows, check_normalisation)

from icl_amd.utils.hashfill import fill_like_reference_init, synthetic_volume  # noqa: E402

pytestmark = pytest.mark.gpu

# The band of tests/test_gpu_parity.py for its fp32 convolution shapes (test_conv3d, lines 48-51): 2e-5 on the forward and the input
# gradient, 1e-4 on the weight and the bias gradient, max |difference| / max |reference|.
CONV_FWD_BAND, CONV_WGRAD_BAND = 2e-5, 1e-4


@pytest.fixture(scope="module")
def dev():
    from icl_amd import _lib
    assert _lib.lib_path().endswith("libicl_hip.so"), "GPU tests must run on the HIP library"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def lib(dev):
    from icl_amd import _lib
    return _lib.lib()


# ---- feed -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("patch", [ref.PATCH_SCALAR, ref.PATCH_QUAD], ids=["scalar", "quad"])
@pytest.mark.parametrize("channels", [1, 2, 3, 4])
def test_feed_sweep_equals_the_forward_chain(dev, lib, channels, patch):
    assert ref.check_sweep(lib, dev, channels, patch) >= 3 * 12 * 2
    if patch == ref.PATCH_QUAD:
        ref.check_sweep(lib, dev, channels, patch, per_launch=5)
        ref.check_sweep(lib, dev, channels, patch, misaligned=True)


def _big_launch(dev, lib, channels, sources, patch, seed):
    rng = np.random.RandomState(seed)
    volumes = [(rng.rand(channels, *s).astype(np.float32) + 0.5, rng.randint(1, 5, size=s).astype(np.uint8)) for s in sources]
    tensors = [(torch.as_tensor(i).to(dev), torch.as_tensor(l).to(dev)) for i, l in volumes]
    from icl_amd.dataloaders.brats2019 import draw_rotflip_crop
    np.random.seed(seed)
    items = [(b % len(sources), tuple(draw_rotflip_crop(sources[b % len(sources)], patch))) for b in range(16)]
    want_image, want_label = ref.expected(volumes, items, patch)
    rc, image, label = ref.raw_channels(lib, tensors, items, channels, patch)
    assert rc == 0
    assert np.array_equal(image.cpu().numpy(), want_image) and np.array_equal(label.cpu().numpy(), want_label)
    ref._KEEP.clear()


def test_feed_full_launch_at_16_x_4_x_16_16_64(dev, lib):
    """Batch 16, C = 4, patch (16, 16, 64) from (20, 18, 64) sources: the depth axis equals the patch's, so the padding rule fires."""
    _big_launch(dev, lib, 4, [(20, 18, 64), (18, 20, 64)], (16, 16, 64), 7)


def test_feed_launch_where_the_grid_stride_loop_wraps(dev, lib):
    """The launcher caps a launch of 16 samples at 128 workgroups a sample (32,768 quads); (32, 34, 128) is 34,816 quads a sample, so
    the first 2,048 threads of every grid row take a second position.  One source needs padding, the other does not."""
    _big_launch(dev, lib, 2, [(40, 38, 130), (30, 30, 100)], (32, 34, 128), 8)


def test_loader_over_a_four_channel_store_equals_the_host_chain(dev):
    from icl_amd.dataloaders.brats2019 import (DeviceVolumeStore, OnDeviceAugment, RandomCrop, RandomRotFlip, ToTensor, draw_rotflip_crop)
    vols = ref.make_store_arrays(4)
    store = DeviceVolumeStore(vols, dev)
    assert store.channels == 4
    for patch in (ref.PATCH_SCALAR, ref.PATCH_QUAD):
        np.random.seed(17)
        got = OnDeviceAugment(store, patch).batch([0, 1, 2, 1])
        assert got["image"].shape == (4, 4, *patch) and got["image"].is_cuda
        np.random.seed(17)
        for j, i in enumerate([0, 1, 2, 1]):
            s = ToTensor()(RandomCrop(patch)(RandomRotFlip()({"image": vols[i][0], "label": vols[i][1]})))
            assert torch.equal(got["image"][j].cpu(), s["image"]) and torch.equal(got["label"][j].cpu(), s["label"])


# ---- intensity and normalisation ---------------------------------------------------------------------------------------------------
# tests/test_gpu_intensity_feed.py grants noise and gamma the bounds of intensity_feed_ref.check_noise / check_gamma against an fp64
# numpy restatement.  No allowance is needed here: both sides of every comparison below are the device's own kernels on the same
# values (the [B,C,...] batch against the same memory viewed as [B C,1,...]), so the equalities of the emulator tests hold bit for bit.

def test_intensity_per_channel_on_the_gpu(dev):
    check_intensity_per_channel(dev)


def test_intensity_shared_rows_on_the_gpu(dev):
    check_intensity_shared_rows(dev)


def test_intensity_one_channel_is_what_it_was_on_the_gpu(dev):
    check_intensity_one_channel_is_unchanged(dev)


@pytest.mark.parametrize("shape,misaligned", [((3, 5, 6, 8), False), ((3, 5, 7, 9), False), ((3, 5, 6, 8), True), ((3, 24, 40, 41), False)])
def test_normalisation_equals_numpy_on_the_gpu(dev, shape, misaligned):
    n = shape[1] * shape[2] * shape[3]      # 1e-12 for fewer than 10^3 additions; the worst case of n additions, n 2^-53, for the large shape
    check_normalisation(dev, shape, std_rel=1e-12 if n < 1000 else n * 2.0 ** -53, misaligned=misaligned)


# ---- first convolution at Cin 2, 3, 4 ----------------------------------------------------------------------------------------------

def _merged_stats(stats):
    """[rows, slots, 3] (count, mean, M2) summaries -> (mean, biased variance) per row, in double (Chan's merge)."""
    s = stats.double().cpu()
    cnt, mean, m2 = s[..., 0], s[..., 1], s[..., 2]
    n = cnt.sum(1)
    mu = (cnt * mean).sum(1) / n
    var = (m2 + cnt * (mean - mu[:, None]) ** 2).sum(1) / n
    return mu, var


@pytest.mark.parametrize("n,cin,d,h,w", [(2, 2, 16, 16, 16), (2, 3, 16, 16, 16), (2, 4, 16, 16, 16), (1, 4, 8, 12, 20)])
def test_first_convolution_with_few_input_channels(dev, n, cin, d, h, w):
    """ops.conv3d at (n, Cin, d, h, w) -> 16 against F.conv3d in fp64 on the CPU: forward, weight gradient, bias gradient, and the
    conv -> InstanceNorm -> ReLU operator whose convolution is asked for the statistics epilogue (want_stats)."""
    from icl_amd import ops
    x = synthetic_volume((n, cin, d, h, w), 1)
    wt = synthetic_volume((16, cin, 3, 3, 3), 2) * (1.0 / np.sqrt(cin * 27))
    b = synthetic_volume((16,), 3) * 0.1
    gy = synthetic_volume((n, 16, d, h, w), 4)
    route = ops.plan_conv3d(x.shape, wt.shape, x_needs_grad=False, has_bias=True, zero_bias_grad=False)
    print("route", cin, (d, h, w), route)
    wd, bd = wt.double().requires_grad_(), b.double().requires_grad_()
    yd = F.conv3d(x.double(), wd, bd, padding=1)
    yd.backward(gy.double())
    wg, bg = wt.to(dev).requires_grad_(), b.to(dev).requires_grad_()
    y = ops.conv3d(x.to(dev), wg, bg)
    y.backward(gy.to(dev))
    errs = (rel_err(y.detach().cpu(), yd.detach()), rel_err(wg.grad.cpu(), wd.grad), rel_err(bg.grad.cpu(), bd.grad))
    print(f"conv3d {cin} -> 16 at {(n, d, h, w)}: fwd {errs[0]:.2e}, wgrad {errs[1]:.2e}, bgrad {errs[2]:.2e}")
    assert errs[0] < CONV_FWD_BAND and errs[1] < CONV_WGRAD_BAND and errs[2] < CONV_WGRAD_BAND
    # the want_stats epilogue: the statistics where the route produces them, and the operator that consumes them
    yy, stats = ops._conv3d_routed(x.to(dev), wt.to(dev), b.to(dev), True, True)
    assert rel_err(yy.cpu(), yd.detach()) < CONV_FWD_BAND
    if stats is not None:
        mu, var = _merged_stats(stats)
        ref_mu, ref_var = yd.detach().flatten(2).mean(2).flatten(), yd.detach().flatten(2).var(2, unbiased=False).flatten()
        scale = float(yd.detach().abs().max())
        assert float((mu - ref_mu).abs().max()) < CONV_FWD_BAND * scale and rel_err(var, ref_var) < 2 * CONV_FWD_BAND
    wn = wt.to(dev).requires_grad_()
    z = ops.conv3d_instance_norm_act(x.to(dev), wn, b.to(dev))
    z.backward(gy.to(dev))
    wnd = wt.double().requires_grad_()
    zd = F.relu(F.instance_norm(F.conv3d(x.double(), wnd, b.double(), padding=1)))
    zd.backward(gy.double())
    e = (rel_err(z.detach().cpu(), zd.detach()), rel_err(wn.grad.cpu(), wnd.grad))
    print(f"conv -> InstanceNorm -> ReLU {cin} -> 16: fwd {e[0]:.2e}, wgrad {e[1]:.2e} (statistics from the epilogue: {stats is not None})")
    assert e[0] < CONV_FWD_BAND and e[1] < CONV_WGRAD_BAND


# ---- the step at in_channels = 4 ---------------------------------------------------------------------------------------------------

def _parity_mode(model):
    from icl_amd.networks.aligner import DropPath
    from icl_amd.networks.layers import Dropout3
    for mod in model.modules():
        if isinstance(mod, Dropout3):
            mod.p = 0.0
        if isinstance(mod, DropPath):
            mod.drop_prob = 0.0


def _small_model(dev):
    from icl_amd.networks.unet_3D_icl import unet_3D_icl
    model = unet_3D_icl(n_classes=ref.STEP_CLASSES, in_channels=ref.STEP_CHANNELS, device=dev, icl_in_resolutions=ref.STEP_RES)
    fill_like_reference_init(list(model.named_parameters()))
    _parity_mode(model)
    return model.train()


def _trainer(model, **kw):
    from icl_amd.trainer import ICLConfig, ICLTrainer
    return ICLTrainer(model, ICLConfig(num_classes=ref.STEP_CLASSES, labeled_bs=1, max_iterations=10, patch_size=ref.STEP_SIZE, **kw))


def test_model_step_with_four_input_channels_matches_the_oracle(dev):
    """unet_3D_icl(n_classes=2, in_channels=4, resolutions (2, 4, 8)) on [2, 4, 32, 32, 32], one labelled and one unlabelled sample,
    against oracle.unet_3d_icl_forward on the CPU: logits within 1e-3, loss terms within 1e-4 (VERDICT, "Precision ruling"); the
    gradient of conv1.conv1.0.weight, the only parameter whose shape is new, against the oracle in fp64 within four times the oracle's own
    fp32-against-fp64 error (multimodal_feed_ref.ORACLE_FP32_GRAD_ERROR)."""
    from icl_amd import ops
    ops.StepRNG.tensor = None
    vol, lab = ref.step_inputs()
    outs32, total32, parts32, _ = ref.oracle_step(torch.float32)
    _, _, _, grad64 = ref.oracle_step(torch.float64)
    model = _small_model(dev)
    tr = _trainer(model)
    outs = model(vol[:1].to(dev), vol[1:].to(dev))
    assert outs[0].shape == (1, 2, 32, 32, 32)
    e_lab, e_unlab = rel_err(outs[0].detach().cpu(), outs32[0].detach()), rel_err(outs[1].detach().cpu(), outs32[1].detach())
    print(f"logits: labelled {e_lab:.2e}, unlabelled {e_unlab:.2e}")
    assert e_lab < 1e-3 and e_unlab < 1e-3
    for name, got_maps, want_maps in (("maps_lab", outs[2], outs32[2]), ("maps_unlab", outs[3], outs32[3]), ("maps_con", outs[4], outs32[4])):
        for i, (g, w) in enumerate(zip(got_maps, want_maps)):
            assert rel_err(g.detach().cpu(), w.detach()) < 1e-3, (name, i)
    loss, parts = tr.compute_loss(outs, lab.to(dev))
    got = [float(parts[k]) for k in ("dice", "ce", "aux", "pse", "con")] + [float(loss)]
    want = [float(parts32[k]) for k in ("dice", "ce", "aux", "pse", "con")] + [float(total32)]
    print("losses", got, want)
    assert np.allclose(got, want, rtol=0, atol=1e-4), (got, want)
    tr.optimizer.zero_grad(set_to_none=True)
    loss.backward()
    g = dict(model.named_parameters())["conv1.conv1.0.weight"].grad
    assert g.shape == (16, 4, 3, 3, 3)
    err = rel_err(g.cpu(), grad64)
    band = ref.GRAD_BAND_FACTOR * ref.ORACLE_FP32_GRAD_ERROR
    print(f"conv1.conv1.0.weight gradient against the fp64 oracle: {err:.3e} (band {band:.3e})")
    assert err < band
    missing = [k for k, p in model.named_parameters() if p.grad is None]
    one = _without_gradient(dev, 1)
    assert missing == one, (missing, one)


def _without_gradient(dev, channels):
    """The parameters that get no gradient in a step of the same small model with `channels` input channels."""
    from icl_amd.networks.unet_3D_icl import unet_3D_icl
    from icl_amd.utils.hashfill import synthetic_labels
    model = unet_3D_icl(n_classes=2, in_channels=channels, device=dev, icl_in_resolutions=ref.STEP_RES)
    fill_like_reference_init(list(model.named_parameters()))
    _parity_mode(model)
    model.train()
    tr = _trainer(model)
    vol = synthetic_volume((2, channels, 32, 32, 32), 1337).to(dev)
    loss, _ = tr.compute_loss(model(vol[:1], vol[1:]), synthetic_labels((1, 32, 32, 32), 4242, 2).to(dev))
    loss.backward()
    return [k for k, p in model.named_parameters() if p.grad is None]


def test_captured_step_with_four_input_channels_equals_eager_steps(dev):
    """ICLTrainer.capture + two replays against eager steps of the same model and batch, with the criterion of
    tests/test_gpu_parity.py::test_graph_replay_equals_eager_steps (lines 922-923): 2 warm-up + 2 replayed steps == 4 eager steps,
    parameters within 1e-5 (max-norm relative), the two losses within 1e-4 relative."""
    from icl_amd import ops
    vol, lab = ref.step_inputs()
    vol, lab = vol.to(dev), lab.to(dev)
    finals = []
    for graphed in (False, True):
        ops.StepRNG.tensor = None
        model = _small_model(dev)
        tr = _trainer(model)
        if graphed:
            tr.capture(vol, lab, warmup=2)
            losses = [tr.step(vol, lab)["loss"].clone() for _ in range(2)]
        else:
            losses = [tr.step(vol, lab)["loss"].clone() for _ in range(4)][2:]
        assert tr.iter_num == 4
        finals.append((model.final.weight.detach().clone(), dict(model.named_parameters())["conv1.conv1.0.weight"].detach().clone(),
                       model.sspa.class_decoders[2].mlp2.fc1.bias.detach().clone(), [float(v) for v in losses]))
        del tr, model
        torch.cuda.empty_cache()
    ops.StepRNG.tensor = None
    (w0, c0, b0, l0), (w1, c1, b1, l1) = finals
    print("eager", l0, "replayed", l1, rel_err(w1.cpu(), w0.cpu()), rel_err(c1.cpu(), c0.cpu()), rel_err(b1.cpu(), b0.cpu()))
    assert rel_err(w1.cpu(), w0.cpu()) < 1e-5 and rel_err(c1.cpu(), c0.cpu()) < 1e-5 and rel_err(b1.cpu(), b0.cpu()) < 1e-5
    assert np.allclose(l0, l1, rtol=1e-4), (l0, l1)


def test_factory_builds_four_channel_nets(dev):
    from icl_amd.networks.net_factory_3d import net_factory_3d
    for net_type in ("unet_3D", "unet_3D_icl"):
        net = net_factory_3d(net_type, in_chns=4, class_num=2)
        assert dict(net.named_parameters())["conv1.conv1.0.weight"].shape == (16, 4, 3, 3, 3) and next(net.parameters()).is_cuda


# ---- SwinUNETR_icl at in_channels = 4 ----------------------------------------------------------------------------------------------

def _lrelu(x):
    return F.leaky_relu(x, 0.01)


def test_swinunetr_icl_with_four_input_channels(dev):
    """PatchEmbed and encoder1 are the two modules that see Cin: each against an fp64 restatement with F.conv3d on the CPU, forward and
    weight gradient, in the band of the convolution test, at feature_size 12; then the whole model's forward and backward (at
    feature_size 48, see below): finite outputs, and a gradient for every parameter that gets one at one input channel."""
    from icl_amd import ops
    from icl_amd.networks.swinunetr_icl import SwinUNETR_icl
    ops.StepRNG.tensor = None

    def build(cin, feature_size):
        m = SwinUNETR_icl(img_size=(32, 32, 32), in_channels=cin, out_channels=2, feature_size=feature_size, device=dev)
        fill_like_reference_init(list(m.named_parameters()))
        _parity_mode(m)
        return m.train()
    model = build(4, 12)
    x = synthetic_volume((2, 4, 32, 32, 32), 5)
    # PatchEmbed: Conv3d(k = 2, s = 2), channels-last tokens
    pe = model.swinViT.patch_embed
    gy = synthetic_volume((2, 16, 16, 16, 12), 6)
    tok = pe(x.to(dev))
    tok.backward(gy.to(dev))
    wd = pe.proj.weight.detach().cpu().double().requires_grad_()
    td = F.conv3d(x.double(), wd, pe.proj.bias.detach().cpu().double(), stride=2).permute(0, 2, 3, 4, 1)
    td.backward(gy.double())
    e = (rel_err(tok.detach().cpu(), td.detach()), rel_err(pe.proj.weight.grad.cpu(), wd.grad))
    print(f"PatchEmbed 4 -> 12: fwd {e[0]:.2e}, wgrad {e[1]:.2e}")
    assert e[0] < CONV_FWD_BAND and e[1] < CONV_WGRAD_BAND
    # encoder1: UnetResBlock(4 -> 12) with the 1x1x1 shortcut
    enc = model.encoder1
    gz = synthetic_volume((2, 12, 32, 32, 32), 7)
    model.zero_grad(set_to_none=True)
    z = enc(x.to(dev))
    z.backward(gz.to(dev))
    names = ("conv1", "conv2", "conv3")
    w64 = {k: getattr(enc.layer, k).conv.weight.detach().cpu().double().requires_grad_() for k in names}
    xd = x.double()
    out = _lrelu(F.instance_norm(F.conv3d(xd, w64["conv1"], padding=1)))
    res = F.instance_norm(F.conv3d(xd, w64["conv3"]))
    zd = _lrelu(F.instance_norm(F.conv3d(out, w64["conv2"], padding=1)) + res)
    zd.backward(gz.double())
    e = [rel_err(z.detach().cpu(), zd.detach())] + [rel_err(getattr(enc.layer, k).conv.weight.grad.cpu(), w64[k].grad) for k in names]
    print("encoder1 4 -> 12: fwd {:.2e}, wgrad conv1 {:.2e}, conv2 {:.2e}, conv3 {:.2e}".format(*e))
    assert e[0] < CONV_FWD_BAND and max(e[1:]) < CONV_WGRAD_BAND
    # the whole model

    def grads(m, cin):
        m.zero_grad(set_to_none=True)
        v = synthetic_volume((2, cin, 32, 32, 32), 8).to(dev)
        outs = m(v[:1], v[1:])
        flat = [outs[0], outs[1], *outs[2], *outs[3], *outs[4]]
        assert all(torch.isfinite(t).all() for t in flat)
        sum((t.float() ** 2).mean() for t in flat).backward()
        got = {k for k, p in m.named_parameters() if p.grad is not None}
        assert all(torch.isfinite(p.grad).all() for p in m.parameters() if p.grad is not None)
        return got
    # (feature_size 12 gives the attention heads a width of 4; the window-attention kernels take 16 or 32 at any channel count, so the
    #  whole model runs at the smallest width they take, feature_size 48, where PatchEmbed and encoder1 see the four channels as well)
    four = grads(build(4, 48), 4)
    one = grads(build(1, 48), 1)
    assert one <= four and "swinViT.patch_embed.proj.weight" in four and "encoder1.layer.conv3.conv.weight" in four


# ---- validation --------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def net2(dev):
    from icl_amd.networks.unet_3D import unet_3D
    model = unet_3D(n_classes=3, in_channels=2, device=dev)
    fill_like_reference_init(list(model.named_parameters()))
    return model.eval()


def _both_ways(monkeypatch, fn):
    out = {}
    for way in ("device", "aten"):
        monkeypatch.setenv("ICL_VAL_WINDOWS", way)
        out[way] = fn()
    return out["device"], out["aten"]


def test_single_case_on_a_two_channel_case_both_ways(dev, net2, monkeypatch):
    """test_single_case_base with a hash-filled unet_3D(n_classes=3, in_channels=2) on a [2, 40, 36, 34] case, patch 32^3, strides 16: the
    kernel form against the ATen form — the score within the 2e-6 that tests/test_gpu_window.py (line 112) grants two soft-maxes
    that differ in their last bits, the label maps equal wherever the two best scores are further apart than that."""
    from icl_amd import val_3D
    image = synthetic_volume((2, 40, 36, 34), 51).numpy()
    (lab_d, score_d), (lab_a, score_a) = _both_ways(monkeypatch, lambda: val_3D.test_single_case_base(
        net2, "unet_3D", image, 16, 16, (32, 32, 32), num_classes=3, return_score=True))
    assert lab_d.shape == lab_a.shape == (40, 36, 34) and score_d.shape == score_a.shape == (3, 40, 36, 34)
    diff = np.abs(score_d - score_a).max()
    top = np.sort(score_a, axis=0)
    clear = (top[-1] - top[-2]) > 4e-6
    print(f"score: largest difference {diff:.3e}; labels that differ: {(lab_d != lab_a).mean():.3e}; clear voxels {clear.mean():.4f}")
    assert diff <= 2e-6 and np.array_equal(lab_d[clear], lab_a[clear])
    assert clear.mean() > 0.5                                       # (of the test itself: most voxels are decided by more than rounding)
    assert len(np.unique(lab_a)) > 1


def test_sliding_window_inference_on_two_channels_both_ways(dev, net2, monkeypatch):
    """The AMOS loop adds logits, the same adds in the same order: equal both ways (the criterion of
    tests/test_gpu_window.py::test_sliding_window_inference_equals_the_aten_loop)."""
    from icl_amd import val_3D
    x = synthetic_volume((1, 2, 40, 32, 45), 52).to(dev)
    got, want = _both_ways(monkeypatch, lambda: val_3D.sliding_window_inference(x, (32, 32, 32), 4, net2))
    assert got.shape == want.shape == (1, 3, 40, 32, 45) and torch.equal(got, want)
    assert torch.isfinite(got).all() and got.std() > 0
