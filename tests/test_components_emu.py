"""CPU checks of the connected-component kernels (icl_amd/csrc/kernels/components.h) through tests/hipemu and the C ABI, against
scipy.ndimage.label.  Cases and reference: tests/components_ref.py.  The emulator runs workgroups on several OS threads, so the
races of the merge kernel are real here too."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hipemu"))
sys.path.insert(0, HERE)
from build_emu import build_emu  # noqa: E402

import components_ref as cr  # noqa: E402
from icl_amd import _lib, ops  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def emu_library():
    _lib._use_library_for_tests(build_emu(), host_pointers=True)
    yield
    _lib._use_library_for_tests(None)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@pytest.mark.parametrize("k", cr.CONNECTIVITIES)
@pytest.mark.parametrize("name", list(cr.CASES))
def test_case(name, k):
    m, nc = cr.CASES[name]()
    labels, counts = ops.seg_components(_t(m), nc, k)
    cr.check_labels(m, labels.numpy(), counts.numpy(), nc, k)
    for keep_largest, min_size in cr.filter_settings(m, nc, k):
        out = ops.seg_filter_components(_t(m), nc, k, keep_largest, min_size)
        cr.check_filter(m, out.numpy(), nc, k, keep_largest, min_size)


def test_what_the_cases_are_about():
    """The cases' own preconditions, on the reference."""
    m, _ = cr.checkerboard()
    assert [cr.ClassReference(m, 1, k).n for k in (1, 2, 3)] == [int(m.sum()), 1, 1]
    m, _ = cr.corner_and_edge()
    assert [cr.ClassReference(m, 1, k).n for k in (1, 2, 3)] == [2, 2, 1]      # the corner joins under 26 neighbours only
    assert [cr.ClassReference(m, 2, k).n for k in (1, 2, 3)] == [2, 1, 1]      # the edge under 18 and 26
    for axis in range(3):
        m, _ = cr.ties(axis)
        assert cr.ClassReference(m, 1, 1).record() == [2, 2, 1]               # two components of two voxels: the first one is "the largest"
    m, _ = cr.two_classes_face_to_face()
    assert [cr.ClassReference(m, c, 3).n for c in (1, 2)] == [1, 1]


@pytest.mark.parametrize("k", cr.CONNECTIVITIES)
def test_ties_keep_the_first(k):
    for axis in range(3):
        m, nc = cr.ties(axis)
        out = ops.seg_filter_components(_t(m), nc, k).numpy()
        assert out.ravel().tolist() == [1, 1, 0, 0, 0]


@pytest.mark.parametrize("k", cr.CONNECTIVITIES)
@pytest.mark.parametrize("dtype", [np.uint8, np.int64])
def test_out_may_be_the_map(k, dtype):
    m, nc = cr.CASES["random_nc4_d5"]()
    m = m.astype(dtype)
    t = _t(m.copy())
    got = ops.seg_filter_components(t, nc, k, True, 0, out=t)
    assert got is t
    cr.check_filter(m, t.numpy(), nc, k, True, 0)


@pytest.mark.parametrize("k", cr.CONNECTIVITIES)
def test_two_runs_are_bit_equal(k):
    m, nc = cr.serpentine()
    a = ops.seg_components(_t(m), nc, k)
    b = ops.seg_components(_t(m), nc, k)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    m, nc = cr.CASES["random_nc17_d8"]()
    a = ops.seg_components(_t(m), nc, k)
    b = ops.seg_components(_t(m), nc, k)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(ops.seg_filter_components(_t(m), nc, k), ops.seg_filter_components(_t(m), nc, k))


def test_bad_arguments_are_refused():
    a = torch.zeros((4, 4, 4), dtype=torch.int64)
    for fn in (ops.seg_components, ops.seg_filter_components):
        for nc in (1, 257):
            with pytest.raises(ValueError):
                fn(a, nc)
        for k in (0, 4, True, 1.0):
            with pytest.raises(ValueError):
                fn(a, 2, k)
        with pytest.raises(ValueError):
            fn(torch.zeros((2, 4, 4, 4), dtype=torch.int64), 2)
        with pytest.raises(ValueError):
            fn(torch.zeros((4, 4), dtype=torch.int64), 2)
        with pytest.raises(TypeError):
            fn(a.float(), 2)
        with pytest.raises(TypeError):
            fn(a.int(), 2)
    for ms in (-1, 1.5, True):
        with pytest.raises(ValueError):
            ops.seg_filter_components(a, 2, 1, True, ms)
    with pytest.raises(ValueError):
        ops.seg_filter_components(a, 2, out=torch.zeros((4, 4, 4), dtype=torch.uint8))
    # the C entry points themselves: -1 with a message, nothing launched (the output buffers stay as they were)
    L = _lib.lib()
    labels = torch.full((64,), 77, dtype=torch.int32)
    counts = torch.full((1, 3), 77, dtype=torch.int64)
    out = torch.full((4, 4, 4), 77, dtype=torch.int64)
    ws = torch.empty(L.icl_seg_components_ws_bytes(4, 4, 4, 2), dtype=torch.uint8)
    null = dict(map=None), dict(labels=None), dict(counts=None), dict(ws=None)
    for kw in (dict(nc=1), dict(nc=257), dict(n0=0), dict(n2=-1), dict(dtype=4), dict(dtype=2), dict(k=0), dict(k=4), dict(k=-1)) + null:
        arg = dict(map=a.data_ptr(), labels=labels.data_ptr(), counts=counts.data_ptr(), ws=ws.data_ptr(), nc=2, n0=4, n2=4, dtype=8, k=1)
        arg.update(kw)
        rc = L.icl_seg_components(arg["map"], arg["dtype"], arg["n0"], 4, arg["n2"], arg["nc"], arg["k"], arg["labels"], arg["counts"],
                                  arg["ws"], None)
        assert rc == -1 and b"seg_components" in L.icl_last_error(), kw
        assert int(labels.min()) == 77 and int(counts.min()) == 77
    null = dict(map=None), dict(out=None), dict(ws=None)
    for kw in (dict(nc=1), dict(nc=257), dict(n0=0), dict(dtype=4), dict(k=0), dict(k=4), dict(ms=-1), dict(ms=-2 ** 62)) + null:
        arg = dict(map=a.data_ptr(), out=out.data_ptr(), ws=ws.data_ptr(), nc=2, n0=4, dtype=8, k=1, ms=0)
        arg.update(kw)
        rc = L.icl_seg_filter_components(arg["map"], arg["dtype"], arg["n0"], 4, 4, arg["nc"], arg["k"], 1, arg["ms"], arg["out"],
                                         counts.data_ptr(), arg["ws"], None)
        assert rc == -1 and b"seg_filter_components" in L.icl_last_error(), kw
        assert int(out.min()) == 77 and int(counts.min()) == 77
    assert L.icl_seg_components_ws_bytes(4, 4, 4, 1) == -1 and L.icl_seg_components_ws_bytes(4, 4, 4, 257) == -1
    assert L.icl_seg_components_ws_bytes(0, 4, 4, 2) == -1
    assert L.icl_seg_components_ws_bytes(1 << 11, 1 << 10, 1 << 10, 2) == -1      # 2^31 voxels: a label would not fit an int32
    # counts may be NULL in the filter
    assert L.icl_seg_filter_components(a.data_ptr(), 8, 4, 4, 4, 2, 1, 1, 0, out.data_ptr(), None, ws.data_ptr(), None) == 0
    assert int(out.max()) == 0


def test_filter_returns_counts_when_asked():
    m, nc = cr.CASES["random_nc4_d5"]()
    t = _t(m)
    L = _lib.lib()
    n0, n1, n2 = m.shape
    ws = torch.empty(L.icl_seg_components_ws_bytes(n0, n1, n2, nc), dtype=torch.uint8)
    out = torch.empty_like(t)
    counts = torch.empty((nc - 1, 3), dtype=torch.int64)
    assert L.icl_seg_filter_components(t.data_ptr(), 1, n0, n1, n2, nc, 2, 0, 3, out.data_ptr(), counts.data_ptr(), ws.data_ptr(), None) == 0
    assert torch.equal(counts, ops.seg_components(t, nc, 2)[1])
    cr.check_filter(m, out.numpy(), nc, 2, False, 3)


def test_host_tensor_is_refused_by_the_product_library():
    _lib._use_library_for_tests(None)
    try:
        a = torch.zeros((4, 4, 4), dtype=torch.int64)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.seg_components(a, 2)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.seg_filter_components(a, 2)
    finally:
        _lib._use_library_for_tests(build_emu(), host_pointers=True)


# the sizes that the library of commit ca1119d2aa3a5921954c12ced9f9332573bd19a7 (the parent of the one that put the workspace carver into the
# launchers) returns, recorded from its emulation build: the layout of the workspace has not moved
@pytest.mark.parametrize("shape, nc, nbytes", [((1, 1, 1), 2, 793344), ((5, 7, 9), 3, 796416), ((3, 300, 2), 256, 814848), ((96, 96, 96), 16, 11409408)])
def test_workspace_size_is_that_of_the_earlier_layout(shape, nc, nbytes):
    assert _lib.lib().icl_seg_components_ws_bytes(*shape, nc) == nbytes
