"""Multi-modal feed (crop_rotflip_channels_kernel and the channel_norm_* kernels in csrc/kernels/datafeed.h, the intensity stage on
[B,C,...] batches, icl_amd/dataloaders/brats2019.py) on the CPU emulation of the kernel sources, against the numpy restatement in
tests/multimodal_feed_ref.py; the GPU run is in test_gpu_multimodal.py.  The gather, the statistics' mean and the applied normalisation
are compared exactly.  Parity with MONAI's own NormalizeIntensityd is unpinned (MONAI is not installed)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "hipemu"))
from build_emu import build_emu  # noqa: E402
import multimodal_feed_ref as ref  # noqa: E402

from icl_amd import _lib  # noqa: E402
from icl_amd.dataloaders.amos import ForegroundIndex, OnDeviceAugmentAMOS, OnDeviceAugmentPosNeg  # noqa: E402
from icl_amd.dataloaders.brats2019 import (DeviceVolumeStore, OnDeviceAugment, RandomCrop, RandomRotFlip, ToTensor,  # noqa: E402
                                           channel_norm_stats, draw_rotflip_crop, normalize_channels_)
from icl_amd.dataloaders.intensity import IntensityAugment  # noqa: E402

CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def emu():
    _lib._use_library_for_tests(build_emu(), host_pointers=True)
    yield _lib.lib()
    _lib._use_library_for_tests(None)


# ---- the gather -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("channels", [1, 2, 3, 4])
def test_scalar_form_sweep_equals_the_forward_chain(emu, channels):
    """Patch (6, 6, 5): one voxel per thread; 3 sources x 4 rotations x 3 flips x the depth origins, 16 mixed samples a launch."""
    assert ref.check_sweep(emu, CPU, channels, ref.PATCH_SCALAR) >= 3 * 12 * 2


@pytest.mark.parametrize("channels", [1, 2, 3, 4])
def test_quad_form_sweep_equals_the_forward_chain(emu, channels):
    """Patch (6, 6, 8): one quad per thread, quad loads where the sources are aligned and inside the row, guarded loads elsewhere."""
    assert ref.check_sweep(emu, CPU, channels, ref.PATCH_QUAD) >= 3 * 12 * 2
    ref.check_sweep(emu, CPU, channels, ref.PATCH_QUAD, per_launch=5)                      # partial launches, other mixes


@pytest.mark.parametrize("channels", [1, 3])
def test_misaligned_image_output_takes_the_scalar_form_and_is_still_equal(emu, channels):
    ref.check_sweep(emu, CPU, channels, ref.PATCH_QUAD, misaligned=True)


def _tensors(channels):
    return [(torch.as_tensor(i), torch.as_tensor(l)) for i, l in ref.make_store_arrays(channels)]


def test_launcher_refuses_bad_arguments_and_writes_nothing(emu):
    tensors = _tensors(2)
    items = ref.sweep_rows(ref.PATCH_QUAD)[:3]
    rc, image, label = ref.raw_channels(emu, tensors, items, 2, ref.PATCH_QUAD)
    assert rc == 0 and not (image == -7).any() and not (label == -7).any()

    def refused(match, items_=items, channels=2, patch=ref.PATCH_QUAD, **kw):
        rc, image, label = ref.raw_channels(emu, tensors, items_, channels, patch, **kw)
        assert rc == -1
        with pytest.raises(RuntimeError, match=match):
            _lib.check(rc, "crop_rotflip_channels")
        assert (image == -7).all() and (label == -7).all()

    for null in range(5):
        refused("null pointer", null=null)
    refused("channels 0 out of range", channels=0, patch=ref.PATCH_QUAD)
    refused("channels 17 out of range", channels=17)
    refused("batch 0 out of range", batch=0)
    refused("batch 17 out of range", items_=(items * 6)[:16], batch=17)
    si, row = items[0]
    refused("bad sample 1", items_=[items[0], (si, row[:3] + (4,) + row[4:])])                    # k = 4
    refused("bad sample 0", items_=[(si, row[:5] + (-1,) + row[6:])])                             # negative padding
    refused("output extents", patch=(6, 6, 0))
    # a null volume pointer inside the pointer arrays
    m = 1
    ptrs = ctypes.c_void_p * m
    out_i, out_l = torch.full((1, 2, *ref.PATCH_QUAD), -7.0), torch.full((1, *ref.PATCH_QUAD), -7, dtype=torch.int64)
    rc = emu.icl_crop_rotflip_channels(ptrs(None), ptrs(tensors[si][1].data_ptr()), (ctypes.c_int32 * 11)(*row), 1, 2, out_i.data_ptr(),
                                       out_l.data_ptr(), *ref.PATCH_QUAD, None)
    assert rc == -1 and b"null volume pointer" in emu.icl_last_error() and (out_i == -7).all() and (out_l == -7).all()


def test_store_keeps_channels_and_refuses_mixed_layouts(emu):
    vols = ref.make_store_arrays(3)
    store = DeviceVolumeStore(vols, "cpu")
    assert store.channels == 3 and store.multichannel and len(store) == 3 and store.images[0].shape == (3, 7, 9, 5)
    flat = DeviceVolumeStore(ref.make_store_arrays(None), "cpu")
    assert flat.channels == 1 and not flat.multichannel
    two = ref.make_store_arrays(2)
    with pytest.raises(ValueError, match="same channels"):
        DeviceVolumeStore([vols[0], two[1]], "cpu")
    with pytest.raises(ValueError, match="same channels"):
        DeviceVolumeStore([vols[0], ref.make_store_arrays(None)[1]], "cpu")
    with pytest.raises(ValueError, match="a volume is"):
        DeviceVolumeStore([(vols[0][0], vols[1][1])], "cpu")                                   # label of other extents
    with pytest.raises(ValueError, match="1 to 16 channels"):
        DeviceVolumeStore([(np.zeros((17, 4, 4, 4), np.float32), np.zeros((4, 4, 4), np.uint8))], "cpu")
    adopted = DeviceVolumeStore.from_device_tensors([torch.as_tensor(v[0]) for v in vols], [torch.as_tensor(v[1]) for v in vols], "cpu")
    assert adopted.channels == 3 and adopted.multichannel
    with pytest.raises(ValueError, match="same channels"):
        DeviceVolumeStore.from_device_tensors([torch.as_tensor(vols[0][0]), torch.as_tensor(two[1][0])],
                                              [torch.as_tensor(vols[0][1]), torch.as_tensor(two[1][1])], "cpu")


def test_amos_feeds_refuse_a_multi_channel_store(emu):
    store = DeviceVolumeStore(ref.make_store_arrays(2), "cpu")
    with pytest.raises(ValueError, match="single-channel"):
        OnDeviceAugmentAMOS(store, (6, 6, 8))
    with pytest.raises(ValueError, match="single-channel"):
        OnDeviceAugmentAMOS(store, (6, 6, 8), affine_prob=1.0, rotate_range=(0.1, 0.1, 0.1))
    with pytest.raises(ValueError, match="single-channel"):
        ForegroundIndex(store)
    flat = DeviceVolumeStore(ref.make_store_arrays(None), "cpu")
    index = ForegroundIndex(flat)
    with pytest.raises(ValueError, match="single-channel"):
        OnDeviceAugmentPosNeg(store, index, (6, 6, 8))


def _host_chain(image, label, patch):
    s = ToTensor()(RandomCrop(patch)(RandomRotFlip()({"image": image, "label": label})))
    return s["image"].numpy(), s["label"].numpy()


@pytest.mark.parametrize("patch", [ref.PATCH_SCALAR, ref.PATCH_QUAD])
def test_loader_batch_equals_the_host_chain(emu, patch):
    """OnDeviceAugment over a [C,W,H,D] store: with draw_rotflip_crop's rows the batch equals RandomRotFlip -> RandomCrop -> ToTensor of
    the host path, channel by channel, from the same seed; and a batch drawn inside batch() equals the one given its rows."""
    vols = ref.make_store_arrays(3)
    store = DeviceVolumeStore(vols, "cpu")
    feed = OnDeviceAugment(store, patch)
    idx = [2, 0, 1, 1, 0]
    np.random.seed(41)
    rows = [draw_rotflip_crop(vols[i][0].shape[-3:], patch) for i in idx]
    got = feed.batch(idx, params=rows)
    assert got["image"].shape == (5, 3, *patch) and got["label"].shape == (5, *patch) and got["label"].dtype == torch.int64
    np.random.seed(41)
    for j, i in enumerate(idx):
        image, label = _host_chain(*vols[i], patch)
        assert image.shape == (3, *patch)
        assert np.array_equal(got["image"][j].numpy(), image) and np.array_equal(got["label"][j].numpy(), label)
    np.random.seed(41)
    drawn = feed.batch(idx)
    assert torch.equal(drawn["image"], got["image"]) and torch.equal(drawn["label"], got["label"])
    with pytest.raises(ValueError, match="names the extents"):
        feed.batch([0], params=[rows[0]])                                                          # the row of another volume


def test_single_channel_store_still_goes_through_the_old_entry(emu, monkeypatch):
    calls = []
    lib = _lib.lib()

    class Spy:
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if name.startswith("icl_crop_rotflip"):
                calls.append(name)
            return fn
    monkeypatch.setattr(_lib, "lib", lambda: Spy())
    flat = DeviceVolumeStore(ref.make_store_arrays(None), "cpu")
    np.random.seed(3)
    out = OnDeviceAugment(flat, ref.PATCH_QUAD).batch([0, 1])
    assert out["image"].shape == (2, 1, *ref.PATCH_QUAD) and calls == ["icl_crop_rotflip"]
    one = DeviceVolumeStore(ref.make_store_arrays(1), "cpu")
    np.random.seed(3)
    out1 = OnDeviceAugment(one, ref.PATCH_QUAD).batch([0, 1])
    assert calls == ["icl_crop_rotflip", "icl_crop_rotflip_channels"]
    assert torch.equal(out1["image"], out["image"]) and torch.equal(out1["label"], out["label"])


# ---- intensity stage --------------------------------------------------------------------------------------------------------------

INTENSITY = dict(noise_prob=0.8, noise_sigma=(0.05, 0.2), noise_clip=2.0, blur_prob=0.6, blur_sigma=(0.5, 0.9), contrast_prob=0.7,
                 gamma_prob=0.7, invert_prob=0.3)
ROI = (6, 6, 8)


def _batch(shape, seed=9):
    return torch.as_tensor(np.random.RandomState(seed).uniform(-1, 3, size=shape).astype(np.float32))


def check_intensity_per_channel(device):
    stage = IntensityAugment(ROI, rng=np.random.RandomState(21), **INTENSITY)
    assert stage.per_channel
    rows = stage.draw(2, channels=3)
    old = IntensityAugment(ROI, rng=np.random.RandomState(21), **INTENSITY)
    assert rows == [r for _ in range(6) for r in old.draw(1)] and len(rows) == 6                   # six consecutive draws of a single row
    assert any(r[0] for r in rows) and any(r[6] or r[8] for r in rows)
    x = _batch((2, 3, *ROI)).to(device)
    got = stage.apply(x.clone(), rows)
    flat = old.apply(x.clone().view(6, 1, *ROI), rows)
    assert got.shape == (2, 3, *ROI) and torch.equal(got.view(torch.int32), flat.view(2, 3, *ROI).view(torch.int32))
    assert stage.stats.shape == (6, 4) and torch.equal(stage.stats, old.stats)
    # rows drawn inside apply: the same stream of draws
    a = IntensityAugment(ROI, rng=np.random.RandomState(21), **INTENSITY).apply(x.clone())
    assert torch.equal(a, got)


def check_intensity_shared_rows(device):
    stage = IntensityAugment(ROI, rng=np.random.RandomState(22), per_channel=False, noise_prob=1.0, noise_sigma=0.3, contrast_prob=1.0)
    rows = stage.draw(2, channels=3)
    assert len(rows) == 2 and all(r[0] == 1 for r in rows)
    x = _batch((2, 3, *ROI)).to(device)
    got = stage.apply(x.clone(), rows)
    per_patch = [r[:1] + ((int(r[1]) + c) % 2 ** 32,) + r[2:] for r in rows for c in range(3)]     # the seed rule
    want = IntensityAugment(ROI, **INTENSITY).apply(x.clone().view(6, 1, *ROI), per_patch).view(2, 3, *ROI)
    assert torch.equal(got, want)
    # the noise fields of two channels of one sample differ: the same data in every channel, noise alone
    noise_only = IntensityAugment(ROI, rng=np.random.RandomState(23), per_channel=False, noise_prob=1.0, noise_sigma=0.3)
    same = _batch((2, 1, *ROI)).expand(2, 3, *ROI).contiguous().to(device)
    out = noise_only.apply(same.clone())
    assert not torch.equal(out[:, 0], out[:, 1]) and not torch.equal(out[:, 1], out[:, 2])
    wrap = noise_only.apply(same.clone(), [(1, 2 ** 32 - 1, 0.3, 0.0) + ref_off_tail()] * 2)        # (seed + c) mod 2^32
    zero = IntensityAugment(ROI, noise_prob=1.0).apply(same[:, :1].clone(), [(1, 0, 0.3, 0.0) + ref_off_tail()] * 2)
    assert torch.equal(wrap[:, 1], zero[:, 0])
    with pytest.raises(ValueError, match="per sample"):
        stage.apply(x.clone(), rows * 3)


def ref_off_tail():
    from icl_amd.dataloaders.intensity import OFF_ROW
    return tuple(OFF_ROW[4:])


def check_intensity_one_channel_is_unchanged(device):
    x = _batch((3, 1, *ROI)).to(device)
    outs, draws = [], []
    for kw in (dict(), dict(per_channel=True), dict(per_channel=False)):
        stage = IntensityAugment(ROI, rng=np.random.RandomState(5), **INTENSITY, **kw)
        rows = stage.draw(3) if not kw else stage.draw(3, channels=1)
        draws.append(rows)
        outs.append(stage.apply(x.clone(), rows))
        assert stage.stats.shape == (3, 4)
    assert draws[0] == draws[1] == draws[2] and torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    four_d = IntensityAugment(ROI, rng=np.random.RandomState(5), **INTENSITY).apply(x.clone().view(3, *ROI), draws[0])
    assert torch.equal(four_d.view(3, 1, *ROI), outs[0])


def test_intensity_per_channel_equals_the_patches_one_by_one(emu):
    check_intensity_per_channel(CPU)


def test_intensity_shared_rows_and_the_seed_rule(emu):
    check_intensity_shared_rows(CPU)


def test_intensity_with_one_channel_is_what_it_was(emu):
    check_intensity_one_channel_is_unchanged(CPU)


def test_loader_draws_intensity_rows_after_the_geometric_rows(emu):
    vols = ref.make_store_arrays(2)
    store = DeviceVolumeStore(vols, "cpu")
    rng = np.random.RandomState(8)
    feed = OnDeviceAugment(store, ROI, intensity=IntensityAugment(ROI, rng=rng, contrast_prob=1.0, noise_prob=1.0))
    np.random.seed(12)
    got = feed.batch([0, 1, 2])
    np.random.seed(12)
    rows = [draw_rotflip_crop(vols[i][0].shape[-3:], ROI) for i in (0, 1, 2)]
    stage = IntensityAugment(ROI, rng=np.random.RandomState(8), contrast_prob=1.0, noise_prob=1.0)
    irows = stage.draw(3, channels=2)
    assert len(irows) == 6
    plain = OnDeviceAugment(store, ROI).batch([0, 1, 2], params=rows)
    want = stage.apply(plain["image"].clone(), irows)
    assert torch.equal(got["image"], want) and torch.equal(got["label"], plain["label"])


# ---- channel-wise normalisation ---------------------------------------------------------------------------------------------------

def check_normalisation(device, shape=(3, 5, 6, 8), std_rel=1e-12, misaligned=False):
    """All three masks and both apply settings on the fixture: the mean equals numpy's float64 mean exactly, the std is within
    `std_rel` of numpy's, the applied volume equals numpy's fp32 evaluation with numpy's own rounded m and s, bit for bit."""
    x = ref.norm_fixture(shape)
    assert not x[1].any() and len(np.unique(x[2][x[2] != 0])) == 1 and (x[0] < 0).any() and (x[0] == 0).any()
    for mask in ref.NORM_MASKS:
        want_stats = ref.norm_reference(x, mask, "mask")[1]
        for c in range(shape[0]):           # no rounding tie: a std within std_rel of numpy's rounds to numpy's fp32 std
            assert want_stats[c, 2] == 0 or ref.no_fp32_tie(want_stats[c, 2], std_rel), (mask, c)
        for apply_to in ref.NORM_APPLY:
            want, _ = ref.norm_reference(x, mask, apply_to)
            if misaligned:
                buf = torch.zeros(x.size + 4, dtype=torch.float32, device=device)
                vol = buf[1:1 + x.size].view(*shape)
                vol.copy_(torch.as_tensor(x))
                assert vol.data_ptr() % 16 == 4
            else:
                vol = torch.as_tensor(x.copy()).to(device)
            stats = channel_norm_stats(vol, mask).cpu().numpy()
            assert stats.shape == (shape[0], 4) and stats.dtype == np.float64
            for c in range(shape[0]):
                assert stats[c, 0] == want_stats[c, 0] and stats[c, 1] == want_stats[c, 1], (mask, c, stats[c], want_stats[c])
                assert abs(stats[c, 2] - want_stats[c, 2]) <= std_rel * want_stats[c, 2], (mask, c, stats[c], want_stats[c])
            out = normalize_channels_(vol, mask, apply_to)
            assert out is vol
            got = vol.cpu().numpy()
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), (mask, apply_to)
            if mask != "all":
                assert np.array_equal(got[1], x[1])                                          # the all-zero channel: untouched
            if apply_to == "mask" and mask == "nonzero":
                assert (got[0][x[0] == 0] == 0).all()                                        # the background stays 0
    single = torch.as_tensor(x[0].copy()).to(device)                                      # a [W,H,D] volume is one channel
    normalize_channels_(single, "positive", "all")
    assert np.array_equal(single.cpu().numpy(), ref.norm_reference(x[:1], "positive", "all")[0][0])


def test_normalisation_equals_numpy(emu):
    check_normalisation(CPU)


def test_normalisation_scalar_loads_and_many_workgroups(emu):
    """Voxel counts that are no multiple of 4, a volume 4 bytes past a 16-byte boundary (one-voxel loads), and (2, 24, 40, 41): 9,840
    groups of four in 39 workgroups a channel, so the finishing kernel has something to add.  The bound on the std is the worst case of
    a sum of N terms, N 2^-53 relative, for the N of the shape."""
    check_normalisation(CPU, (3, 5, 7, 9), std_rel=1e-12)
    check_normalisation(CPU, (3, 5, 6, 8), std_rel=1e-12, misaligned=True)
    big = (3, 24, 40, 41)
    check_normalisation(CPU, big, std_rel=24 * 40 * 41 * 2.0 ** -53)


def test_normalisation_refuses_bad_arguments(emu):
    x = torch.zeros((2, 4, 4, 4))
    for bad in (x.double(), x.numpy(), x.transpose(2, 3), torch.zeros((4, 4)), torch.zeros((17, 2, 2, 2))):
        with pytest.raises(ValueError):
            normalize_channels_(bad)
    with pytest.raises(ValueError, match="mask"):
        normalize_channels_(x, mask="foreground")
    with pytest.raises(ValueError, match="apply_to"):
        normalize_channels_(x, apply_to="some")
    stats, ws = torch.zeros((2, 4), dtype=torch.float64), torch.zeros(2 * 256 * 2, dtype=torch.float64)
    L = _lib.lib()
    for args, match in (((None, 2, 64, 0, stats.data_ptr(), ws.data_ptr(), None), b"null pointer"),
                        ((x.data_ptr(), 2, 64, 0, None, ws.data_ptr(), None), b"null pointer"),
                        ((x.data_ptr(), 0, 64, 0, stats.data_ptr(), ws.data_ptr(), None), b"channels 0"),
                        ((x.data_ptr(), 17, 64, 0, stats.data_ptr(), ws.data_ptr(), None), b"channels 17"),
                        ((x.data_ptr(), 2, 0, 0, stats.data_ptr(), ws.data_ptr(), None), b"voxels"),
                        ((x.data_ptr(), 2, 64, 3, stats.data_ptr(), ws.data_ptr(), None), b"mask mode 3")):
        assert L.icl_channel_norm_stats(*args) == -1 and match in L.icl_last_error()
    assert L.icl_channel_norm_apply(x.data_ptr(), 2, 64, 0, 2, stats.data_ptr(), None) == -1 and b"apply mode 2" in L.icl_last_error()
    assert L.icl_channel_norm_apply(x.data_ptr(), 2, 64, 0, 0, None, None) == -1
    assert not x.any()
    _lib._use_library_for_tests(None)                    # the product binding refuses host memory before any pointer travels
    try:
        with pytest.raises(ValueError, match="HIP device"):
            normalize_channels_(x)
    finally:
        _lib._use_library_for_tests(build_emu(), host_pointers=True)
