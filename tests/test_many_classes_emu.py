"""More than 16 classes through the training kernels, on the kernel emulation (tests/hipemu): the generic-class loss path
(csrc/kernels/loss.h, 17 .. 256 classes) and the class tiles of the prototype attention (token.h).  The cases, references and bands
are those of tests/many_classes_ref.py; tests/test_gpu_many_classes.py runs the same on the device."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hipemu"))
from build_emu import build_emu  # noqa: E402

import many_classes_ref as M  # noqa: E402
from icl_amd import _lib, ops  # noqa: E402

CPU = torch.device("cpu")


@pytest.fixture(scope="module", autouse=True)
def emu_library():
    _lib._use_library_for_tests(build_emu(), host_pointers=True)
    yield
    _lib._use_library_for_tests(None)


@pytest.mark.parametrize("nc,S,scale", M.LOSS_CASES)
def test_losses_beyond_16_classes_match_torch(nc, S, scale):
    M.check_losses(nc, S, scale, CPU)


def test_all_loss_terms_in_one_launch_beyond_16_classes():
    """ops.fused_losses at 17 classes: the multi entry points on the generic-class kernels, against torch and bit-equal to the
    term-by-term calls (job j of the multi kernels is launch j of the single ones), twice."""
    nc, S = 17, (6, 8, 10)
    multi = M.run_multi(nc, S, CPU, single=False)
    again = M.run_multi(nc, S, CPU, single=False)
    single = M.run_multi(nc, S, CPU, single=True)
    assert multi[0] == again[0] == single[0]
    for a, b, c in zip(multi[1], again[1], single[1]):
        assert torch.equal(a, b) and torch.equal(a, c)
    M.assert_multi_close(multi, M.multi_reference(nc, S), "fused_losses nc=17")


@pytest.mark.parametrize("nc", [2, 3, 16])
def test_forced_generic_path_agrees_with_the_register_path(monkeypatch, nc):
    """ICL_LOSS_GENERIC=1 sends any class count through the generic-class kernels: within the bands of the register path's results on
    the same inputs, single-term and multi, and both within the bands of torch."""
    S = (6, 5, 7)
    monkeypatch.delenv("ICL_LOSS_GENERIC", raising=False)
    reg, reg_multi = M.run_losses(nc, S, 1.0, CPU), M.run_multi(nc, S, CPU, single=False)
    monkeypatch.setenv("ICL_LOSS_GENERIC", "1")
    gen, gen2 = M.run_losses(nc, S, 1.0, CPU), M.run_losses(nc, S, 1.0, CPU)
    gen_multi, gen_multi2 = M.run_multi(nc, S, CPU, single=False), M.run_multi(nc, S, CPU, single=False)
    M.assert_bit_equal(gen, gen2, f"generic nc={nc}")
    assert gen_multi[0] == gen_multi2[0] and all(torch.equal(a, b) for a, b in zip(gen_multi[1], gen_multi2[1]))
    M.assert_losses_close(gen, reg, f"generic vs register nc={nc}")
    M.assert_losses_close(gen, M.loss_reference(nc, S, 1.0), f"generic vs torch nc={nc}")
    M.assert_multi_close(gen_multi, reg_multi, f"generic vs register, multi, nc={nc}")
    M.assert_multi_close(gen_multi, M.multi_reference(nc, S), f"generic vs torch, multi, nc={nc}")


def test_257_classes_are_refused_and_nothing_is_launched():
    nc, B, S = 257, 1, 8
    a, lab = torch.zeros(B, nc, S), torch.zeros(B, S, dtype=torch.int64)
    for call in (lambda: ops.cross_entropy_dice_parts(a, lab, nc), lambda: ops.soft_dice_loss(a, a.clone()),
                 lambda: ops.fused_losses([(a, lab, 1), (a, a.clone(), 3)]),
                 lambda: ops.prototype_attention(torch.zeros(1, 2, nc, 8), torch.zeros(1, 5, 32), 2, 1.0)):
        with pytest.raises(ValueError, match="256"):
            call()
    # the C ABI itself: -1, a message naming the limit, outputs untouched
    L = _lib.lib()
    stats = torch.full(((3 * nc + 1) * (1 + ops.LOSS_MAX_BLOCKS),), -7.0)
    out, ga = torch.full((2,), -7.0), torch.full((B, nc, S), -7.0)
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    assert L.icl_loss_fwd(p(a), None, p(lab), None, p(stats), p(out), B, nc, S, 1, 0, None) == -1
    assert b"256" in L.icl_last_error()
    assert L.icl_loss_bwd(p(a), None, p(lab), None, p(stats), None, p(out), p(ga), B, nc, S, 1, 0, None) == -1
    assert b"256" in L.icl_last_error()
    job = ops._LossJob()
    job.a, job.labels, job.stats, job.out, job.ga = a.data_ptr(), lab.data_ptr(), stats.data_ptr(), out.data_ptr(), ga.data_ptr()
    job.s, job.batch, job.nc, job.mode = S, B, nc, 1
    for fn in (L.icl_loss_fwd_multi, L.icl_loss_bwd_multi):
        assert fn(ctypes.byref(job), 1, None) == -1 and b"256" in L.icl_last_error()
    q, kv = torch.zeros(1, 2, nc, 8), torch.zeros(1, 5, 32)
    lg, o, st = torch.full((1, nc, 2, 5), -7.0), torch.full((1, 2, nc, 8), -7.0), torch.full((1, 2, nc, 2), -7.0)
    assert L.icl_attn_fwd(p(q), p(kv), p(lg), p(o), p(st), 1, 2, nc, 5, 8, 1.0, None) == -1 and b"256" in L.icl_last_error()
    gq, gkv = torch.full_like(q, -7.0), torch.full_like(kv, -7.0)
    assert L.icl_attn_bwd_ws(p(q), p(kv), p(lg), p(st), p(o), p(o), None, p(gq), p(gkv), None, 1, 2, nc, 5, 8, 1.0, None) == -1
    assert b"256" in L.icl_last_error()
    for t in (stats, out, ga, lg, o, st, gq, gkv):
        assert bool((t == -7.0).all())
    # a call of jobs from two class groups is refused as before
    jobs = (ops._LossJob * 2)()
    for j, k in enumerate((16, 17)):
        jobs[j].a, jobs[j].labels, jobs[j].stats, jobs[j].out = a.data_ptr(), lab.data_ptr(), stats.data_ptr(), out.data_ptr()
        jobs[j].s, jobs[j].batch, jobs[j].nc, jobs[j].mode = S, B, k, 1
    assert L.icl_loss_fwd_multi(jobs, 2, None) == -1 and b"17 .. 256" in L.icl_last_error()


@pytest.mark.parametrize("B,h,nc,d,N", M.ATTN_CASES)
def test_prototype_attention_beyond_16_classes(B, h, nc, d, N):
    M.check_attention(B, h, nc, d, N, CPU)


@pytest.mark.parametrize("tag,train", [("tr", True), ("ev", False)])
def test_small_aligner_at_17_classes_matches_reference_golden(tag, train):
    from conftest import load_golden
    M.check_aligner(CPU, load_golden("many_classes.npz"), tag, train)


@pytest.mark.parametrize("B,h,nc,d,N", M.ATTN_SMALL_CASES)
def test_forced_class_tiles_agree_with_the_single_tile_kernels(monkeypatch, B, h, nc, d, N):
    """ICL_ATTN_TILED=1 sends any class count through the class-tiled logits and dK / dV kernels: within the bands of torch and of the
    single-tile kernels' results on the same inputs."""
    monkeypatch.delenv("ICL_ATTN_TILED", raising=False)
    plain = M.run_attention(B, h, nc, d, N, CPU)
    monkeypatch.setenv("ICL_ATTN_TILED", "1")
    M.check_attention(B, h, nc, d, N, CPU)
    M.check_attention(B, h, nc, d, N, CPU, against=plain)
