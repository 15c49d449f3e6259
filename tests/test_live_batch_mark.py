"""The live-batch mark (icl_amd/ops.py mark_live / live_of, DESIGN.md §4.4 "Live batch") on the CPU: the helper alone, its way through autograd, and
the operators that read it on the CPU emulation of the same kernels (tests/hipemu) at small shapes — the MI355X cases are in
tests/test_gpu_live_batch.py."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hipemu"))
from build_emu import build_emu  # noqa: E402

import live_batch_checks as C  # noqa: E402
from icl_amd import _lib, ops  # noqa: E402

# Weight / bias gradients of a live run keep the slab plan of the full batch (the workgroups that own no live tile are skipped and their
# slabs written as zeros): bitwise equality, no band.
EMU_BAND = None


@pytest.fixture(scope="module")
def emu_library():
    _lib._use_library_for_tests(build_emu(), host_pointers=True)
    yield
    _lib._use_library_for_tests(None)


# ---- the helper alone --------------------------------------------------------------------------------------------------------------

def test_mark_reads_back_and_an_inplace_write_voids_it(monkeypatch):
    monkeypatch.setenv("ICL_LIVE_BATCH", "1")
    g = torch.zeros(3, 2, 4)
    g[:2] = 1.0
    assert ops.live_of(g, 3) is None
    assert ops.mark_live(g, 2) is g and ops.live_of(g, 3) == 2
    g.add_(torch.ones_like(g))          # autograd accumulating into a stolen buffer: the tail is no longer zero
    assert ops.live_of(g, 3) is None
    ops.mark_live(g, 1)
    assert ops.live_of(g, 3) == 1
    g[2:].zero_()                       # any in-place write counts, whatever it wrote
    assert ops.live_of(g, 3) is None


def test_views_slices_and_copies_do_not_inherit_the_mark(monkeypatch):
    monkeypatch.setenv("ICL_LIVE_BATCH", "1")
    g = ops.mark_live(torch.zeros(4, 6, 2), 1)
    assert ops.live_of(g, 4) == 1
    for v in (g[:, :3], g[:2], g.view(4, 12), g.view_as(g), g.detach(), g.clone(), g.reshape(4, 3, 4), g * 1.0):
        assert ops.live_of(v, v.shape[0]) is None
    assert g.contiguous() is g and ops.live_of(g.contiguous(), 4) == 1      # (what every backward does first: the same object)
    # a write through a view voids the base's mark as well: they share the version counter
    g[:, :3].add_(1.0)
    assert ops.live_of(g, 4) is None


def test_full_empty_and_mismatched_batches_read_as_full(monkeypatch):
    monkeypatch.setenv("ICL_LIVE_BATCH", "1")
    for k in (0, 3, 5, -1, None):       # k == 0, k == n, beyond n: nothing to mark
        g = ops.mark_live(torch.zeros(3, 2), k)
        assert ops.live_of(g, 3) is None and not hasattr(g, ops._LIVE_ATTR)
    g = ops.mark_live(torch.zeros(3, 2), 1)
    assert ops.live_of(g, 3) == 1 and ops.live_of(g, 2) is None and ops.live_of(g, 4) is None      # another leading dimension
    assert ops.live_of(None, 3) is None and ops.mark_live(None, 1) is None
    assert ops.live_of(ops.mark_live(torch.zeros(()), 1), 1) is None                                # a scalar has no batch


def test_the_switch_never_marks(monkeypatch):
    monkeypatch.setenv("ICL_LIVE_BATCH", "0")
    g = ops.mark_live(torch.zeros(3, 2), 1)
    assert not hasattr(g, ops._LIVE_ATTR) and ops.live_of(g, 3) is None
    monkeypatch.setenv("ICL_LIVE_BATCH", "1")
    ops.mark_live(g, 1)
    monkeypatch.setenv("ICL_LIVE_BATCH", "0")          # read per call: a mark made before the switch is not trusted either
    assert ops.live_of(g, 3) is None


class _Probe(torch.autograd.Function):
    seen = []

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        _Probe.seen.append(ops.live_of(g, g.shape[0]))
        return g


def test_split_batch_is_the_producer_and_the_mark_crosses_autograd_nodes(monkeypatch):
    """_SplitBatch.backward marks when the second half has no gradient and the first has one — not in the reverse case, not when both
    have one; the mark arrives at the next Function's backward (the same tensor object), and not behind an ATen op or an accumulation."""
    monkeypatch.setenv("ICL_LIVE_BATCH", "1")

    def grads_seen(use_a, use_b, through=lambda t: t):
        _Probe.seen.clear()
        x = torch.randn(3, 4, 2, requires_grad=True)
        a, b = ops.split_batch(through(_Probe.apply(x)), 1)
        loss = (a.sum() * 2 if use_a else 0) + (b.sum() * 3 if use_b else 0)
        loss.backward()
        return list(_Probe.seen), x.grad
    seen, g = grads_seen(True, False)
    assert seen == [1] and int(torch.count_nonzero(g[1:])) == 0 and bool((g[:1] == 2).all())
    assert grads_seen(False, True)[0] == [None]          # live suffix: out of scope, today's path
    assert grads_seen(True, True)[0] == [None]
    assert grads_seen(True, False, through=lambda t: t * 1.0)[0] == [None]      # an ATen op between: a new tensor, full batch
    # two consumers of one tensor: autograd adds the gradients, the sum carries no mark
    _Probe.seen.clear()
    x = torch.randn(3, 4, requires_grad=True)
    p = _Probe.apply(x)
    a, _ = ops.split_batch(p, 2)
    (a.sum() + p.sum()).backward()
    assert _Probe.seen == [None] and bool((x.grad[2:] == 1).all())
    monkeypatch.setenv("ICL_LIVE_BATCH", "0")
    assert grads_seen(True, False)[0] == [None]


# ---- the operators on the emulated kernels -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("lazy,w", [(False, 8), (False, 6), (True, 8)])
def test_skip_and_pool_skips_the_dead_addend(emu_library, monkeypatch, k, lazy, w):
    """maxpool2_bwd_add_x2_kernel (rows that pool to an even width) / maxpool2_bwd_add_kernel (w = 6 -> 3) with skip_live: the skip
    gradient is the marked channel-slice view of the concat gradient, the pooling gradient is a full batch; x's gradient is bit for
    bit the full run's in every sample.  The up-sampling backward (`deep`) runs on the live samples."""
    res = C.run_pair(monkeypatch, C.skip_pool_case("cpu", 3, 3, 2, 4, 6, w, lazy), k)
    C.compare(res, k, batched={"deep"}, full={"x"})
    assert ((3, 3, 4, 6, w), k) in res["marks"] and ((3, 2, 2, 3, w // 2), k) in res["marks"]      # the skip view and gdeep


@pytest.mark.parametrize("k", [1, 2])
def test_deferred_norm_backward_on_the_live_samples(emu_library, monkeypatch, k):
    res = C.run_pair(monkeypatch, C.lazy_norm_case("cpu", 3, 5, 3, 4, 8), k)
    C.compare(res, k, batched={"y"})
    assert res["marks"] == [((3, 5, 3, 4, 8), k)] * 2          # _SplitBatch's, then _NormActLazy's on its input gradient


@pytest.mark.parametrize("k", [1, 2])
def test_conv_norm_chain_on_the_live_samples(emu_library, monkeypatch, k):
    """_Conv3d (split-product input gradient and weight gradient) + _NormAct at a small volume the split-product kernels take."""
    monkeypatch.setenv("ICL_CONV_SPLIT_MIN", "1")
    res = C.run_pair(monkeypatch, C.conv_norm_case("cpu", 3, 32, 16, 4, 8, 16), k)
    rep = []
    C.compare(res, k, batched={"x"}, band=EMU_BAND, report=rep)
    print("live-batch deviation (emulated 32->16):", rep)
    assert ((3, 32, 4, 8, 16), k) in res["marks"]          # the input gradient went out marked: the live path ran
    launched, planned = res["wgrad_grid"]
    assert 0 < launched < planned, (launched, planned)     # ... and the weight gradient skipped the workgroups without a live tile


def test_conv_off_the_split_product_kernels_runs_the_full_batch(emu_library, monkeypatch):
    """A volume below the split-product kernels' threshold: the fp32 launchers plan by the batch size, so the convolution reads the
    whole (really zero-tailed) gradient — same numbers as the parent, no mark on its input gradient."""
    res = C.run_pair(monkeypatch, C.conv_norm_case("cpu", 3, 8, 4, 3, 4, 8), 1)
    C.compare(res, 1, batched={"x"})                                     # weights bit for bit too
    assert res["marks"] == [((3, 4, 3, 4, 8), 1)] * 2                    # _SplitBatch's and _NormAct's; none from _Conv3d ([3, 8, ...])


@pytest.mark.parametrize("k", [1, 2])
def test_upcat_conv_chain_on_the_live_samples(emu_library, monkeypatch, k):
    monkeypatch.setenv("ICL_CONV_SPLIT_MIN", "1")
    res = C.run_pair(monkeypatch, C.upcat_case("cpu", 3, 16, 16, 16, 4, 8, 16), k)
    C.compare(res, k, batched={"skip", "deep"}, band=EMU_BAND)
    assert ((3, 16, 2, 4, 8), k) in res["marks"] and ((3, 32, 4, 8, 16), k) in res["marks"]


@pytest.mark.parametrize("p,lazy,w", [(0.3, True, 64), (0.3, False, 64), (0.0, True, 64), (0.3, True, 32), (0.0, False, 32)])
def test_final_layer_on_the_live_samples(emu_library, monkeypatch, p, lazy, w):
    """The fused `final` layer (n * S >= 65,536; w = 32: the live sample alone is below that — it still runs the full batch's kernel):
    same dropout mask on the live samples (a hash of the element index, and the live samples are a prefix), zeros behind them."""
    res = C.run_pair(monkeypatch, C.final_case("cpu", 3, 4, 2, 32, 32, w, p, lazy), 1)
    C.compare(res, 1, batched={"t"}, band=EMU_BAND)
    assert ((3, 4, 32, 32, w), 1) in res["marks"]
