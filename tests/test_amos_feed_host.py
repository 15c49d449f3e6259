"""Host side of the AMOS data feed (icl_amd/dataloaders/amos.py): the documented order and number of the random draws, the store's
label conversion, the loader, the compat import.  No kernel runs here except through the CPU emulation in the loader test."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "hipemu"))
from build_emu import build_emu  # noqa: E402
import amos_feed_ref as ref  # noqa: E402

from icl_amd import _lib  # noqa: E402
from icl_amd.dataloaders.amos import AMOSDeviceLoader, OnDeviceAugmentAMOS, amos_volume_store, draw_amos_params  # noqa: E402
from icl_amd.dataloaders.brats2019 import TwoStreamBatchSampler  # noqa: E402


def replay(shape, roi, rng, flip_prob=0.10, rot_prob=0.10, max_k=3, shift_offset=0.10, shift_prob=0.50, scale_factor=0.0, scale_prob=0.0):
    """The documented draw order, written out call by call."""
    size, origin = [], []
    for a in range(3):
        size.append(min(roi[a], shape[a]))
        origin.append(int(rng.randint(0, shape[a] - size[a] + 1)) if shape[a] > size[a] else 0)
    left = [(roi[a] - size[a]) // 2 for a in range(3)]
    f0 = rng.rand() < flip_prob
    f1 = rng.rand() < flip_prob
    f2 = rng.rand() < flip_prob
    k = 0
    if rng.rand() < rot_prob:
        k = int(rng.randint(max_k)) + 1
    mul = np.float32(1)
    if scale_prob > 0:
        if rng.rand() < scale_prob:
            mul = np.float32(1 + rng.uniform(-scale_factor, scale_factor))
    add = np.float32(0)
    if rng.rand() < shift_prob:
        add = np.float32(rng.uniform(-shift_offset, shift_offset))
    return (*shape, *origin, *size, *left, int(f0) | int(f1) << 1 | int(f2) << 2, k, float(mul), float(add))


def same_state(a, b):
    sa, sb = a.get_state(), b.get_state()
    return sa[0] == sb[0] and np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]


# 0, 1 and 3 axes not larger than the ROI (96^3): no randint for those axes
SHAPES = [(130, 101, 97), (200, 96, 120), (60, 96, 95)]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kw", [{}, {"flip_prob": 0.5, "rot_prob": 0.5, "shift_prob": 0.5},
                                {"flip_prob": 1.0, "rot_prob": 1.0, "shift_prob": 1.0, "max_k": 2, "shift_offset": 0.25},
                                {"rot_prob": 0.0, "shift_prob": 0.0},
                                {"scale_prob": 0.5, "scale_factor": 0.1, "rot_prob": 0.5}])
def test_draws_follow_the_documented_order_and_consume_the_same_state(shape, kw):
    roi = (96, 96, 96)
    seen_k, seen_add, seen_mul = set(), set(), set()
    for seed in range(40):
        a, b = np.random.RandomState(seed), np.random.RandomState(seed)
        got, want = draw_amos_params(shape, roi, a, **kw), replay(shape, roi, b, **kw)
        assert got == want and len(got) == 16, (seed, got, want)
        assert same_state(a, b), seed                                    # the number of draws consumed
        assert all(isinstance(v, int) for v in got[:14]) and all(isinstance(v, float) for v in got[14:])
        assert got[15] == float(np.float32(got[15])) and got[14] == float(np.float32(got[14]))
        seen_k.add(got[13] != 0)
        seen_add.add(got[15] != 0.0)
        seen_mul.add(got[14] != 1.0)
        for ax in range(3):
            n, c, s, left = got[ax], got[3 + ax], got[6 + ax], got[9 + ax]
            assert s == min(96, n) and 0 <= c <= n - s and left == (96 - s) // 2
            if n <= 96:
                assert c == 0
    if kw.get("rot_prob") == 0.5:
        assert seen_k == {True, False}                                    # both outcomes of the coin were replayed
    if kw.get("shift_prob", 0.5) == 0.5:
        assert seen_add == {True, False}
    assert seen_mul == ({True, False} if kw.get("scale_prob") else {False})


def test_draw_counts_are_what_the_order_says():
    """Counted directly on a recording generator: a volume not larger than the ROI on any axis with all coins failing draws five
    rand() and nothing else (three flips, rotation, shift; the scale coin is not even tossed at scale_prob = 0), six with a scale
    probability; with all coins succeeding every conditional draw follows its coin."""
    class Recorder:
        def __init__(self, coin):
            self.calls, self.coin = [], coin

        def rand(self):
            self.calls.append("rand")
            return self.coin

        def randint(self, *a, **k):
            self.calls.append("randint")
            return 0

        def uniform(self, lo, hi):
            self.calls.append("uniform")
            return 0.5 * (lo + hi)

    r = Recorder(0.99)
    draw_amos_params((60, 96, 95), (96, 96, 96), r)
    assert r.calls == ["rand"] * 5
    r = Recorder(0.99)
    draw_amos_params((60, 96, 95), (96, 96, 96), r, scale_prob=0.5, scale_factor=0.1)
    assert r.calls == ["rand"] * 6
    r = Recorder(0.0)
    row = draw_amos_params((100, 96, 97), (96, 96, 96), r, scale_prob=0.5, scale_factor=0.1)
    assert r.calls == ["randint", "randint", "rand", "rand", "rand", "rand", "randint", "rand", "uniform", "rand", "uniform"]
    assert row[12] == 7 and row[13] == 1
    with pytest.raises(ValueError):
        draw_amos_params((60, 96), (96, 96, 96))
    with pytest.raises(TypeError):
        OnDeviceAugmentAMOS(None, (96, 96, 96), flip_probability=0.1)


def test_global_numpy_generator_is_the_default():
    np.random.seed(11)
    got = draw_amos_params((130, 101, 97), (96, 96, 96))
    assert got == replay((130, 101, 97), (96, 96, 96), np.random.RandomState(11))


def test_odd_rotation_on_a_non_square_roi_raises_before_any_launch():
    """The library is not even loaded: the binding would raise `not found` / the launcher would be reached otherwise."""
    image, label = ref.source_volume((9, 7, 8))
    store = amos_volume_store([(image, label)], "cpu")
    with pytest.raises(ValueError, match="rot_prob=0"):
        OnDeviceAugmentAMOS(store, (6, 5, 5))
    feed = OnDeviceAugmentAMOS(store, (6, 5, 5), rot_prob=0.0)
    calls = []
    real = _lib.lib
    _lib.lib = lambda: calls.append(1) or real()
    try:
        for k in (1, 3):
            with pytest.raises(ValueError, match="odd quarter turn"):
                feed.batch([0], params=[ref.make_row((9, 7, 8), (6, 5, 5), (0, 0, 0), 0, k)])
        with pytest.raises(ValueError, match="parameter row for extents"):
            feed.batch([0], params=[ref.make_row((9, 7, 9), (6, 5, 5), (0, 0, 0), 0, 0)])
        with pytest.raises(ValueError, match="16 values"):
            feed.batch([0], params=[(1, 2, 3)])
    finally:
        _lib.lib = real
    assert not calls


def test_store_converts_float_labels_and_rejects_what_is_no_label():
    image = np.linspace(0, 1, 4 * 5 * 6, dtype=np.float32).reshape(1, 4, 5, 6)
    label = (np.arange(4 * 5 * 6) % 16).astype(np.float32).reshape(1, 4, 5, 6)
    label[0, 0, 0, 0] = 255.0
    store = amos_volume_store([{"image": image, "label": label}, {"image": torch.from_numpy(image), "label": torch.from_numpy(label)},
                               (image[0], label[0].astype(np.int16))], "cpu")
    assert len(store) == 3
    for i in range(3):
        assert store.images[i].dtype == torch.float32 and store.labels[i].dtype == torch.uint8
        assert store.images[i].shape == store.labels[i].shape == (4, 5, 6)
        assert np.array_equal(store.images[i].numpy(), image[0]) and np.array_equal(store.labels[i].numpy(), label[0].astype(np.uint8))
    bad = label.copy()
    bad[0, 1, 2, 3] = 2.5
    with pytest.raises(ValueError, match="fractional"):
        amos_volume_store([{"image": image, "label": bad}], "cpu")
    bad[0, 1, 2, 3] = np.nan
    with pytest.raises(ValueError, match="fractional or non-finite"):
        amos_volume_store([{"image": image, "label": bad}], "cpu")
    for value in (256.0, -1.0):
        bad[0, 1, 2, 3] = value
        with pytest.raises(ValueError, match="outside 0..255"):
            amos_volume_store([{"image": image, "label": bad}], "cpu")
    with pytest.raises(ValueError, match="one channel"):
        amos_volume_store([{"image": np.zeros((2, 4, 5, 6), np.float32), "label": np.zeros((2, 4, 5, 6), np.float32)}], "cpu")
    with pytest.raises(ValueError, match="one extent"):
        amos_volume_store([{"image": image, "label": label[:, :3]}], "cpu")
    # DeviceVolumeStore itself is unchanged: it still casts whatever it is given
    from icl_amd.dataloaders.brats2019 import DeviceVolumeStore
    assert DeviceVolumeStore([(image[0], np.full((4, 5, 6), 2.5, np.float32))], "cpu").labels[0].unique().tolist() == [2]


def test_loader_yields_the_samplers_batches():
    _lib._use_library_for_tests(build_emu(), host_pointers=True)
    try:
        shapes = [ref.SOURCES[i % 3] for i in range(10)]
        store = amos_volume_store([ref.source_volume(s) for s in shapes], "cpu")
        roi = ref.ROI_QUAD
        rng = np.random.RandomState(5)
        feed = OnDeviceAugmentAMOS(store, roi, rng=rng, flip_prob=0.5, rot_prob=0.5)
        np.random.seed(21)
        sampler = TwoStreamBatchSampler(list(range(4)), list(range(4, 10)), 4, 2)
        loader = AMOSDeviceLoader(feed, sampler)
        assert len(loader) == len(sampler) == 2
        np.random.seed(21)
        want_batches = [list(map(int, b)) for b in TwoStreamBatchSampler(list(range(4)), list(range(4, 10)), 4, 2)]
        replay_rng = np.random.RandomState(5)
        np.random.seed(21)
        count = 0
        for i_batch, sampled_batch in enumerate(loader):
            idx = want_batches[i_batch]
            rows = [draw_amos_params(shapes[i], roi, replay_rng, flip_prob=0.5, rot_prob=0.5) for i in idx]
            assert sampled_batch["image"].shape == (4, 1, *roi) and sampled_batch["label"].shape == (4, 1, *roi)
            assert sampled_batch["label"].dtype == torch.int64
            for j, (i, row) in enumerate(zip(idx, rows)):
                wi, wl = ref.forward_chain(*ref.source_volume(shapes[i]), row, roi)
                assert np.array_equal(sampled_batch["image"][j].numpy(), wi) and np.array_equal(sampled_batch["label"][j].numpy(), wl)
            lab = sampled_batch["label"][:2].squeeze(1).long()               # the trainer's expressions (:225-227)
            assert lab.shape == (2, *roi) and sampled_batch["label"][:2].long().shape == (2, 1, *roi)
            count += 1
        assert count == len(loader)
    finally:
        _lib._use_library_for_tests(None)


def test_compat_root_resolves_the_amos_feed_import():
    code = ("from dataloaders.amos import AMOSDeviceLoader, OnDeviceAugmentAMOS, amos_volume_store\n"
            "from dataloaders.brats2019 import TwoStreamBatchSampler\n"
            "import icl_amd.dataloaders.amos as a\n"
            "assert AMOSDeviceLoader is a.AMOSDeviceLoader and OnDeviceAugmentAMOS is a.OnDeviceAugmentAMOS\n"
            "assert amos_volume_store is a.amos_volume_store\n"
            "print('compat ok')\n")
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "compat") + os.pathsep + ROOT, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd="/tmp", timeout=300)
    assert out.returncode == 0 and "compat ok" in out.stdout, out.stdout + out.stderr
