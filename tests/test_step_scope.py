"""ops.StepScope: one object owns the state of an open training step (icl_amd/step_scope.py).  However a step ends — its update, an
exception in forward or backward, ``abandon_step()``, the death of the optimiser that opened it — nothing of it is left behind; the two
owners (ICLTrainer, FusedSGD) never open two scopes at once.  On the emulator library (tests/hipemu), small instance of the real model."""
import gc
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hipemu"))
from build_emu import build_emu  # noqa: E402
from icl_amd import _lib, ops  # noqa: E402
from icl_amd.networks.layers import BatchNormAct  # noqa: E402
from icl_amd.networks.unet_3D_icl import unet_3D_icl  # noqa: E402
from icl_amd.optim import FusedSGD, tag_model_parameters  # noqa: E402
from icl_amd.trainer import ICLConfig, ICLTrainer  # noqa: E402
from icl_amd.utils.hashfill import synthetic_labels, synthetic_volume  # noqa: E402

NC = 2


@pytest.fixture(scope="module", autouse=True)
def emu_library():
    _lib._use_library_for_tests(build_emu(), host_pointers=True)
    old_min = ops.FactoredGrads.min_elems
    ops.FactoredGrads.min_elems = 64 * 64          # the 64-token mlp2 matrices of the finest scale stay factored
    yield
    ops.FactoredGrads.min_elems = old_min
    _lib._use_library_for_tests(None)


def _model():
    torch.manual_seed(7)
    model = tag_model_parameters(unet_3D_icl(feature_scale=16, n_classes=NC, in_channels=1, icl_in_resolutions=(1, 2, 4), icl_heads=(8, 4, 2)))
    for m in model.modules():           # no dropout / drop-path randomness between the runs that are compared
        if hasattr(m, "p") and m.__class__.__name__ == "Dropout3":
            m.p = 0.0
        if hasattr(m, "drop_prob"):
            m.drop_prob = 0.0
    return model


def _trainer(model):
    return ICLTrainer(model, ICLConfig(num_classes=NC, labeled_bs=1, patch_size=(16, 16, 16), base_lr=0.05, weight_decay=1e-2))


VOL = synthetic_volume((2, 1, 16, 16, 16), 900)
LAB = synthetic_labels((2, 16, 16, 16), 950, NC)


def _bare_grads():
    """Plain forward / backward of a bare module that has every kind of layer a step scope treats specially: convolutions (packed
    weights, lane, deferred slab sums), BatchNorm (deferred counter), an owner-Linear above FactoredGrads.min_elems (factored
    gradient, deferred bias gradient) and a LayerNorm (deferred partial sums)."""
    from icl_amd.networks.aligner import Linear
    from icl_amd.networks.layers import Conv3d
    torch.manual_seed(3)
    conv, bn, lin = Conv3d(2, 4, 3), BatchNormAct(4, 1), Linear(64, 64)
    ln_w, ln_b = torch.nn.Parameter(torch.ones(64) * 1.5), torch.nn.Parameter(torch.zeros(64) + 0.25)
    x = synthetic_volume((1, 2, 4, 4, 4), 11)
    y = ops.layer_norm(lin(bn(conv(x)).flatten(2)), ln_w, ln_b)
    (y * synthetic_volume(tuple(y.shape), 12)).sum().backward()
    params = [conv.weight, conv.bias, bn.weight, bn.bias, lin.weight, lin.bias, ln_w, ln_b]
    assert all(p.grad is not None and not getattr(p, "_icl_factors", None) for p in params)      # dense, complete, now
    assert int(bn.num_batches_tracked) == 1
    return [p.grad.clone() for p in params]


@pytest.fixture(scope="module")
def fresh(emu_library):
    """What a process that never opened a step computes."""
    assert ops.StepScope.current is None
    return _bare_grads()


def _assert_at_rest(fresh):
    assert ops.StepScope.current is None and BatchNormAct.deferred is None and ops.PackedWeights.current is None
    assert not ops.FactoredGrads.enabled and ops.FactoredGrads.fused_optimizer is None and ops.FactoredGrads.uses is None
    assert ops.WgradLane.uses is None and not ops.WgradLane.open and ops.DeferredBiasGrads.pending is None
    assert ops.DeferredWgradReduce.pending is None
    got = _bare_grads()
    assert all(torch.equal(a, b) for a, b in zip(got, fresh))


class _Boom(RuntimeError):
    pass


def _raise(*a):
    raise _Boom("injected")


@pytest.mark.timeout(1200)
def test_trainer_step_leaves_nothing_behind_however_it_ends(fresh):
    model = _model()
    tr = _trainer(model)
    tr.step(VOL, LAB[:1])
    _assert_at_rest(fresh)
    # forward raises (inside the aligners: packed weights, counters and use counts are in flight)
    h = model.uscl.register_forward_pre_hook(_raise)
    with pytest.raises(_Boom):
        tr.step(VOL, LAB[:1])
    h.remove()
    _assert_at_rest(fresh)
    # backward raises (half-way: gradients are queued on the deferrals)
    h = model.center.register_full_backward_hook(_raise)
    with pytest.raises(_Boom):
        tr.step(VOL, LAB[:1])
    h.remove()
    _assert_at_rest(fresh)
    tr.step(VOL, LAB[:1])              # ... and the trainer steps on
    _assert_at_rest(fresh)


def _loss(model):
    from icl_amd.utils import losses
    outputs = model(VOL[:1], VOL[1:])
    return (losses.DiceLoss(NC)(torch.softmax(outputs[0], 1), LAB[:1].unsqueeze(1)) + torch.nn.CrossEntropyLoss()(outputs[0], LAB[:1])
            + 10 * losses.softmax_mse_loss(outputs[3], outputs[4]))


@pytest.mark.timeout(1200)
def test_fused_sgd_scope_leaves_nothing_behind_however_it_ends(fresh):
    model = _model()
    opt = FusedSGD(model.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-2)
    # closed by step()
    loss = _loss(model)
    scope = ops.StepScope.current
    assert scope is not None and scope.owner() is opt and ops.FactoredGrads.enabled
    opt.zero_grad()
    loss.backward()
    assert ops.StepScope.current is scope          # the scope outlives backward
    opt.step()
    _assert_at_rest(fresh)
    # closed by abandon_step()
    _loss(model).backward()
    assert ops.StepScope.current is not None
    opt.abandon_step()
    _assert_at_rest(fresh)
    # the owner is garbage-collected while its scope is open
    _loss(model)
    assert ops.StepScope.current is not None and ops.StepScope.current.owner() is opt
    del opt, loss, scope
    gc.collect()
    _assert_at_rest(fresh)


@pytest.mark.timeout(1200)
def test_fused_sgd_hook_inside_a_trainer_step_opens_no_second_scope():
    """A model that carries FusedSGD's forward pre-hook, stepped by an ICLTrainer: the hook fires while the trainer's scope is open
    and leaves it alone; the step equals that of a model without the hook, bit for bit."""
    def run(hooked):
        model = _model()
        other = FusedSGD(model.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-2) if hooked else None
        tr = _trainer(model)
        seen = []
        model.register_forward_pre_hook(lambda *a: seen.append(ops.StepScope.current))      # (registered after FusedSGD's: fires after it)
        parts = [tr.step(VOL, LAB[:1]) for _ in range(2)]
        assert len(seen) == 2 and all(s is not None and s.owner() is None and s.packed is tr.packed for s in seen)
        assert ops.StepScope.current is None
        if hooked:
            assert not other._updated_in_backward and not other._scope_packed
        return [float(p["loss"]) for p in parts], {k: p.detach().clone() for k, p in model.named_parameters()}

    (la, a), (lb, b) = run(False), run(True)
    assert la == lb
    assert all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.timeout(1200)
def test_second_training_forward_before_step_raises_only_after_an_update_in_backward(monkeypatch):
    # (the size threshold of the one-pass input gradient + update is the 13,824^2 matrices'; lowered to this model's 64^2 ones)
    monkeypatch.setattr(FusedSGD, "can_update_in_backward",
                        lambda self, p, rows: rows <= 32 and p.numel() >= 64 * 64 and id(p) in self._group_of())
    model = _model()
    opt = FusedSGD(model.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-2)
    _loss(model).backward()
    assert opt._updated_in_backward
    with pytest.raises(RuntimeError, match=r"a training forward pass started after a backward pass that already applied this step's "
                                           r"update of the\s+token-axis matrices \(update_in_backward=True\) and before optimizer.step\(\)"):
        model(VOL[:1], VOL[1:])
    opt.abandon_step()
    assert ops.StepScope.current is None
    # without an update inside backward the second forward joins the open step: one scope, use counts and factors accumulate
    model = _model()
    opt = FusedSGD(model.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-2, update_in_backward=False)
    _loss(model).backward()
    scope = ops.StepScope.current
    mlp2 = [p for k, p in model.named_parameters() if "mlp2" in k and getattr(p, "_icl_factors", None)]
    assert mlp2 and all(len(p._icl_factors) == 1 for p in mlp2)
    _loss(model).backward()
    assert ops.StepScope.current is scope and all(len(p._icl_factors) == 2 for p in mlp2)
    assert max(scope.weight_uses.values()) >= 2
    opt.step()
    assert ops.StepScope.current is None and all(not p._icl_factors for p in mlp2)
