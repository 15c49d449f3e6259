"""SwinUNETR stochastic depth / dropout / in-kernel attention dropout on the device: the dropout instantiations of the window-attention
kernels and one whole block against explicit-mask fp64 (tests/swin_dropout_ref.py; bands of tests/test_gpu_generic.py: 1e-5 outputs,
1e-4 gradients), bit-reproducible trainer steps with the rates on, and hipGraph capture / replay of such a step."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import swin_dropout_ref as R  # noqa: E402
from conftest import rel_err  # noqa: E402
from icl_amd.utils.hashfill import fill_like_reference_init, synthetic_labels, synthetic_volume  # noqa: E402

pytestmark = pytest.mark.gpu

RATES = dict(dropout_path_rate=0.2, drop_rate=0.1, attn_drop_rate=0.1)


@pytest.fixture(scope="module")
def dev():
    from icl_amd import _lib
    assert _lib.lib_path().endswith("libicl_hip.so"), "GPU tests must run on the HIP library"
    return torch.device("cuda", 0)


@pytest.fixture(autouse=True)
def _no_step_rng_left_behind():
    from icl_amd import ops
    ops.StepRNG.tensor = None
    yield
    ops.StepRNG.tensor = None


# ------------------------------------------------------------------------------------------------ 6. kernels and block on the device
@pytest.mark.parametrize("windows,heads,shifted,online", [(16, 3, True, "1"), (8, 6, False, "1"), (8, 12, True, "1"), (2, 24, False, "1"),
                                                          (16, 3, True, "2"), (8, 6, False, "2")])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_window_attention_dropout_343_tokens(dev, monkeypatch, windows, heads, shifted, online, p):
    """343-token windows with the 3 / 6 / 12 / 24 heads of the 96^3 model's four stages, on the register-resident forward (<22, 16, true>;
    what the launcher picks below 512 workgroups) and on the online-soft-max forward (ICL_WINATTN_ONLINE=2 forces it at this size; the
    trainer tests below run it at the model's own 686 x 3 windows)."""
    from icl_amd.networks import swinunetr as SW
    monkeypatch.setenv("ICL_WINATTN_ONLINE", online)
    from oracle import swin_oracle as S
    n, c = 343, heads * 16
    regions = SW.window_regions((14, 14, 14), (7, 7, 7), (3, 3, 3), "cpu") if shifted else None      # 8 windows
    assert regions is None or windows % regions.shape[0] == 0
    qkv = synthetic_volume((windows, n, 3 * c), 71) * 1.5
    table = synthetic_volume((2197, heads), 72)
    gy = synthetic_volume((windows, n, c), 73)
    eo, eq, et = R.check_attention(dev, qkv, table, S.relative_position_index(), regions, heads, 0.25, gy, p, 4242 + heads, rel_err)
    assert eo < 1e-5 and eq < 1e-4 and et < 1e-4


@pytest.mark.parametrize("n,dh,heads,nw,batch,masked", [(49, 32, 2, 4, 3, True), (90, 32, 2, 2, 1, True), (216, 16, 3, 1, 2, False),
                                                        (96, 16, 1, 2, 3, False), (64, 16, 2, 4, 2, True), (100, 16, 2, 1, 3, False),
                                                        (200, 16, 3, 2, 2, True), (300, 16, 2, 3, 1, False)])
def test_window_attention_dropout_other_templates(dev, n, dh, heads, nw, batch, masked):
    """Head dim 32 (2-D Swin-UNet windows: 49 tokens -> <6, 32, false>, 90 -> <6, 32, true>) and the other key-block templates, filled
    (216 -> <14, 16, true>, 96 -> <6, 16, true>) and general (64 / 100 / 200 / 300 tokens -> <6 / 14 / 14 / 22, 16, false>; 300 = 19 of 22 key blocks), as
    test_gpu_generic.py covers them without dropout: with the 343-token test above every dropout instantiation of the library runs."""
    g = torch.Generator().manual_seed(n)
    side = 2 * 7 - 1
    table = synthetic_volume((side ** 3, heads), 172)
    index = torch.randint(0, side ** 3, (343, 343), generator=g)
    regions = torch.randint(0, 3, (nw, n), generator=g).to(torch.int32) if masked else None
    qkv = synthetic_volume((batch * nw, n, 3 * heads * dh), 171) * 1.5
    gy = synthetic_volume((batch * nw, n, heads * dh), 173)
    eo, eq, et = R.check_attention(dev, qkv, table, index, regions, heads, dh ** -0.5, gy, 0.3, 99 + n, rel_err)
    assert eo < 1e-5 and eq < 1e-4 and et < 1e-4


@pytest.mark.parametrize("base", [0, (1 << 32) - 256, (7 << 32) + 99])
def test_keep_decisions_use_the_64_bit_index(dev, base):
    """tests/test_swin_dropout.py's check of the hoisted hash (high word, carry) on the device, with the step counter."""
    from icl_amd import ops
    count, seed, p = 1 << 17, 0xC0FFEE, 0.3
    seed_dev = torch.full((1,), 4, dtype=torch.int32, device=dev)
    got = ops.window_attention_keep_probe(seed_dev, base, count, seed, p, seed_dev)
    assert np.array_equal(got.cpu().numpy(), ops.dropout_keep_mask(seed, count, p, step=4, start=base))


def test_window_attention_rate_zero_is_bit_identical(dev):
    from icl_amd import ops
    from oracle import swin_oracle as S
    heads, n, c = 3, 343, 48
    qkv, table = synthetic_volume((16, n, 3 * c), 71).to(dev), synthetic_volume((2197, heads), 72).to(dev)
    index = S.relative_position_index().to(dev)
    assert torch.equal(ops.window_attention(qkv, table, index, None, heads, 0.25),
                       ops.window_attention(qkv, table, index, None, heads, 0.25, attn_drop=0.0))


@pytest.mark.parametrize("shift,grid", [((3, 3, 3), (8, 8, 8)), ((0, 0, 0), (4, 8, 4))])
def test_block_with_all_rates_matches_explicit_mask_composition(dev, shift, grid):
    """tests/test_swin_dropout.py's block test on the device (head dim 16: c = 48, 3 heads)."""
    errs, dropped_exact = R.check_block(dev, shift, grid, rel_err, c=48, heads=3)
    assert dropped_exact
    assert errs["out"] < 1e-5 and errs["x1"] < 1e-5
    bad = {k: v for k, v in errs.items() if k.startswith("d") and v > 1e-4}
    assert not bad, bad


def test_factory_builds_with_dropout_path_rate(dev):
    from icl_amd.networks import net_factory_3d as F3
    old = F3.args.dropout_path_rate
    try:
        F3.args.dropout_path_rate = 0.2
        m = F3.net_factory_3d("swinunetr_icl", 1, 2)
    finally:
        F3.args.dropout_path_rate = old
    probs = [b.drop_path.drop_prob for i in range(1, 5) for b in getattr(m.swinViT, "layers%d" % i)[0].blocks]
    assert probs == [x.item() for x in torch.linspace(0, 0.2, 8)]


def test_eval_model_ignores_the_rates(dev):
    from icl_amd import ops
    from icl_amd.networks.swinunetr_icl import SwinUNETR_icl
    kw = dict(img_size=(96, 96, 96), in_channels=1, out_channels=2, feature_size=48, device=dev)
    a, b = SwinUNETR_icl(**kw), SwinUNETR_icl(**kw, **RATES)
    fill_like_reference_init(list(a.named_parameters()))
    b.load_state_dict(a.state_dict())
    a.eval(), b.eval()
    vol = synthetic_volume((2, 1, 96, 96, 96), 93).to(dev)
    drawn = []
    real = ops._step_seed
    ops._step_seed = lambda *args: drawn.append(1) or real(*args)
    state = torch.get_rng_state()
    try:
        with torch.no_grad():
            ya, yb = a(vol, inference=True), b(vol, inference=True)
    finally:
        ops._step_seed = real
    assert not drawn and torch.equal(state, torch.get_rng_state())
    assert torch.equal(ya, yb)


# ------------------------------------------------------------------------------------------------ 7. bit-reproducible steps
def _build(dev, rates, seed=20241003):
    from icl_amd import ops
    from icl_amd.networks.swinunetr_icl import SwinUNETR_icl
    ops.StepRNG.tensor = None
    torch.manual_seed(seed)
    model = SwinUNETR_icl(img_size=(96, 96, 96), in_channels=1, out_channels=2, feature_size=48, device=dev, **rates)
    fill_like_reference_init(list(model.named_parameters()))
    model.train()
    return model


def _state(model, tr):
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    for k, p in model.named_parameters():
        if p in tr.optimizer.state and "momentum_buffer" in tr.optimizer.state[p]:
            state["momentum " + k] = tr.optimizer.state[p]["momentum_buffer"].clone()
    return state


def test_steps_with_the_rates_on_are_bit_reproducible(dev):
    """The pattern of test_gpu_parity.py::test_swinunetr_icl_steps_are_bit_reproducible with all three rates on: the masks are a function
    of (torch.manual_seed, call order), nothing is summed atomically; another seed draws other masks."""
    from icl_amd.trainer import ICLConfig, ICLTrainer
    vol = synthetic_volume((2, 1, 96, 96, 96), 93).to(dev)
    lab = synthetic_labels((1, 96, 96, 96), 94, 2).to(dev)
    runs = []
    for seed in (20241003, 20241003, 777):
        model = _build(dev, RATES, seed)
        tr = ICLTrainer(model, ICLConfig(num_classes=2, labeled_bs=1, max_iterations=10))
        losses = [tr.step(vol, lab)["loss"].clone() for _ in range(2)]
        runs.append((losses, _state(model, tr)))
        del tr, model
        torch.cuda.empty_cache()
    (la, sa), (lb, sb), (lc, _) = runs
    print("losses", [float(x) for x in la], [float(x) for x in lb], [float(x) for x in lc])
    assert all(torch.equal(x, y) for x, y in zip(la, lb)), (la, lb)
    differ = [k for k in sa if not torch.equal(sa[k], sb[k])]
    assert not differ, differ[:10]
    assert not any(torch.equal(x, y) for x, y in zip(la, lc)), (la, lc)


# ------------------------------------------------------------------------------------------------ 8. capture and replay
def _aligner_drop_paths_off(model):
    """The aligners' own DropPath (0.1 schedule) off, the backbone's sites untouched: only the new sites can move the loss."""
    from icl_amd.networks.aligner import DropPath
    for name, mod in model.named_modules():
        if isinstance(mod, DropPath) and not name.startswith("swinViT."):
            mod.drop_prob = 0.0


def _captured_run(dev, rates, cfg_kw, replays=3, prepare=None):
    from icl_amd.trainer import ICLConfig, ICLTrainer
    vol = synthetic_volume((2, 1, 96, 96, 96), 93).to(dev)
    lab = synthetic_labels((1, 96, 96, 96), 94, 2).to(dev)
    model = _build(dev, rates)
    if prepare is not None:
        prepare(model)
    tr = ICLTrainer(model, ICLConfig(num_classes=2, labeled_bs=1, max_iterations=10, **cfg_kw))
    tr.capture(vol, lab, warmup=2)
    losses = [tr.step(vol, lab)["loss"].clone() for _ in range(replays)]
    torch.cuda.synchronize()
    state = _state(model, tr)
    del tr, model
    torch.cuda.empty_cache()
    return losses, state


def test_captured_steps_with_rates_are_reproducible(dev):
    """(a) Two captured runs (drop path 0.2, attention dropout 0.1) from the same seed and state: bit-identical losses and weights over
    three replays."""
    rates = dict(dropout_path_rate=0.2, attn_drop_rate=0.1)
    (la, sa), (lb, sb) = _captured_run(dev, rates, {}), _captured_run(dev, rates, {})
    print("replayed losses", [float(x) for x in la])
    assert all(torch.equal(x, y) for x, y in zip(la, lb)), (la, lb)
    differ = [k for k in sa if not torch.equal(sa[k], sb[k])]
    assert not differ, differ[:10]


@pytest.mark.parametrize("rates,moves", [(dict(dropout_path_rate=0.2, drop_rate=0.1, attn_drop_rate=0.1), True),
                                         (dict(attn_drop_rate=0.1), True), (dict(), False)])
def test_replays_draw_new_masks_at_every_new_site(dev, rates, moves):
    """(b) Learning rate 0, weight decay 0, the aligners' DropPath off: the weights stand still, so the three replayed losses differ iff
    a backbone site draws a new mask per replay through the device counter — all sites, the in-kernel one alone, and none."""
    losses, _ = _captured_run(dev, rates, dict(base_lr=0.0, weight_decay=0.0), prepare=_aligner_drop_paths_off)
    vals = [float(x) for x in losses]
    print("replayed losses at lr 0", rates, vals)
    if moves:
        assert len(set(vals)) > 1, vals
    else:
        assert all(torch.equal(losses[0], x) for x in losses[1:]), vals


def _all_rates_off(model):
    """What _parity_mode of test_gpu_parity.py does, plus the attention rate."""
    from icl_amd.networks.aligner import DropPath
    from icl_amd.networks.layers import Dropout3
    from icl_amd.networks.swinunetr import WindowAttention
    for mod in model.modules():
        if isinstance(mod, Dropout3):
            mod.p = 0.0
        if isinstance(mod, DropPath):
            mod.drop_prob = 0.0
        if isinstance(mod, WindowAttention):
            mod.attn_drop = 0.0


def test_graph_replay_equals_eager_steps_with_every_rate_switched_off(dev):
    """(c) A model BUILT with the rates, every drop_prob / p / attention rate then set to 0 on the modules: two eager + two replayed steps
    equal four eager steps within the bands of test_gpu_parity.py::test_graph_replay_equals_eager_steps."""
    from icl_amd.trainer import ICLConfig, ICLTrainer
    vol = synthetic_volume((2, 1, 96, 96, 96), 93).to(dev)
    lab = synthetic_labels((1, 96, 96, 96), 94, 2).to(dev)
    finals = []
    for graphed in (False, True):
        model = _build(dev, RATES)
        _all_rates_off(model)
        tr = ICLTrainer(model, ICLConfig(num_classes=2, labeled_bs=1, max_iterations=10))
        if graphed:
            tr.capture(vol, lab, warmup=2)
            losses = [tr.step(vol, lab)["loss"].clone() for _ in range(2)]
        else:
            losses = [tr.step(vol, lab)["loss"].clone() for _ in range(4)][2:]
        assert tr.iter_num == 4
        sd = model.state_dict()
        finals.append(({k: sd[k].detach().clone() for k in ("out.conv.conv.weight", "swinViT.layers1.0.blocks.1.attn.relative_position_bias_table",
                                                           "swinViT.layers4.0.blocks.0.mlp.linear1.weight")}, [float(x) for x in losses]))
        del tr, model
        torch.cuda.empty_cache()
    (w0, l0), (w1, l1) = finals
    for k in w0:
        e = rel_err(w1[k].cpu(), w0[k].cpu())
        print("eager vs replay", k, e)
        assert e < 1e-5, (k, e)
    print("losses", l0, l1)
    assert np.allclose(l0, l1, rtol=1e-4), (l0, l1)
