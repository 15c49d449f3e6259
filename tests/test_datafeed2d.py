"""2-D data feed and slice resize against vectors generated from the real reference
(tests/golden/make_golden_datafeed2d.py): the host `RandomGenerator`, the fused on-device one (slice_augment_kernel in
csrc/kernels/datafeed.h, here on the CPU emulation of the kernel sources; the GPU run is in test_gpu_datafeed2d.py), the batched
nearest-neighbour resize of the 2-D validation loop, the sampler and the `compat/` import.  Every comparison is exact: these are
gathers."""
import os
import random
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "hipemu"))
sys.path.insert(0, os.path.join(HERE, "golden"))
from build_emu import build_emu  # noqa: E402
from make_golden_datafeed2d import SAMPLER_CASES, ZOOM_CASES, case_slice, digest, zoom_edge_is_zero, zoom_input  # noqa: E402

from icl_amd import _lib  # noqa: E402
from icl_amd.dataloaders.dataset import (BRANCH_NONE, BRANCH_ROTATE, BRANCH_ROTFLIP, DeviceSliceStore, OnDeviceAugment2D,  # noqa: E402
                                         RandomGenerator, TwoStreamBatchSampler, draw_generator, resize_slices, rotate_matrix,
                                         zoom_factor)

GOLD = np.load(os.path.join(HERE, "golden", "datafeed2d.npz"))
SMALL = [tuple(int(v) for v in GOLD[f"small.{n}.cfg"]) for n in range(int(GOLD["small.count"][0]))]   # n0 n1 o0 o1 seed branch k axis angle
REAL = [tuple(int(v) for v in GOLD[f"real.{n}.cfg"]) for n in range(int(GOLD["real.count"][0]))]       # n0 n1 o0 o1 seed


@pytest.fixture(scope="module")
def emu_library():
    _lib._use_library_for_tests(build_emu(), host_pointers=True)
    yield
    _lib._use_library_for_tests(None)


def seed_both(seed):
    random.seed(seed)
    np.random.seed(seed)


def next_draws():
    return np.array([random.random(), float(np.random.randint(0, 1 << 30))])


def assert_digest(a, prefix, gold=GOLD):
    crc, total, sub = digest(np.asarray(a))
    assert np.array_equal(sub, gold[f"{prefix}.sub"]), prefix
    assert int(crc[0]) == int(gold[f"{prefix}.crc"][0]) and float(total[0]) == float(gold[f"{prefix}.sum"][0]), prefix


def test_the_golden_set_covers_what_it_was_searched_for():
    """Every (k, axis) on a non-square slice, the four kinds of angle, the plain branch, up- and downsampling, patch == extent, and
    zero-edge zooms (one in the rotate branch)."""
    rotflips = {(k, axis) for n0, n1, _, _, _, branch, k, axis, _ in SMALL if branch == BRANCH_ROTFLIP and n0 != n1}
    assert rotflips == {(k, axis) for k in range(4) for axis in range(2)}
    angles = [angle for *_, branch, _, _, angle in SMALL if branch == BRANCH_ROTATE]
    assert 0 in angles and -20 in angles and any(-20 < a < 0 for a in angles) and any(a > 0 for a in angles)
    assert any(branch == BRANCH_NONE for *_, branch, _, _, _ in SMALL)
    assert any(o0 > n0 for n0, _, o0, *_ in SMALL) and any(o0 < n0 for n0, _, o0, *_ in SMALL)
    assert any((n0, n1) == (o0, o1) for n0, n1, o0, o1, *_ in SMALL)
    edge = []
    for n0, n1, o0, o1, _, branch, k, _, _ in SMALL:
        r0, r1 = (n1, n0) if branch == BRANCH_ROTFLIP and k & 1 else (n0, n1)
        if zoom_edge_is_zero(r0, o0) or zoom_edge_is_zero(r1, o1):
            edge.append(branch)
    assert len(edge) >= 2 and BRANCH_ROTATE in edge
    assert {draw_after_seed(c[4]) for c in REAL} == {BRANCH_NONE, BRANCH_ROTFLIP, BRANCH_ROTATE}


def draw_after_seed(seed):
    seed_both(seed)
    return draw_generator((8, 8), (8, 8))[2]


def test_host_random_generator_equals_the_reference():
    for n, (n0, n1, o0, o1, seed, *_) in enumerate(SMALL):
        image, label = case_slice((n0, n1), seed)
        seed_both(seed)
        s = RandomGenerator([o0, o1])({"image": image, "label": label})
        assert s["image"].dtype == torch.float32 and s["label"].dtype == torch.uint8 and set(s) == {"image", "label"}
        assert s["image"].shape == (1, o0, o1) and s["label"].shape == (o0, o1)
        assert np.array_equal(s["image"].numpy(), GOLD[f"small.{n}.image"]), n
        assert np.array_equal(s["label"].numpy(), GOLD[f"small.{n}.label"]), n
        assert np.array_equal(next_draws(), GOLD[f"small.{n}.next"]), n


def test_draw_generator_follows_the_reference_call_sequence():
    """Branch, k, axis and angle as recorded with the goldens; both generators end where the reference's call leaves them; the
    rotation record is scipy's matrix and offset, the zoom factors are (r - 1) / (o - 1) of the extents after rot90."""
    for n, (n0, n1, o0, o1, seed, branch, k, axis, angle) in enumerate(SMALL):
        seed_both(seed)
        rec = draw_generator((n0, n1), (o0, o1))
        assert np.array_equal(next_draws(), GOLD[f"small.{n}.next"]), n
        assert len(rec) == 13 and rec[:3] == (n0, n1, branch), n
        r0, r1 = n0, n1
        if branch == BRANCH_ROTFLIP:
            assert rec[3:5] == (k, axis)
            r0, r1 = (n1, n0) if k & 1 else (n0, n1)
        if branch == BRANCH_ROTATE:
            assert rec[5:11] == rotate_matrix((n0, n1), angle)
        assert rec[11:] == ((r0 - 1) / (o0 - 1), (r1 - 1) / (o1 - 1))
    with pytest.raises(AssertionError):
        zoom_factor(3, 2 ** 60 + 1)          # an extent pair for which scipy would not produce the asked output extent
    with pytest.raises(ValueError):
        zoom_factor(8, 1)


def check_small_cases(device):
    slices = [case_slice(c[:2], c[4]) for c in SMALL]
    store = DeviceSliceStore(slices, device)
    assert len(store) == len(SMALL)
    for n, (n0, n1, o0, o1, seed, *_) in enumerate(SMALL):
        seed_both(seed)
        out = OnDeviceAugment2D(store, (o0, o1)).batch([n])
        assert out["image"].shape == (1, 1, o0, o1) and out["image"].dtype == torch.float32
        assert out["label"].shape == (1, o0, o1) and out["label"].dtype == torch.uint8
        assert np.array_equal(out["image"][0].cpu().numpy(), GOLD[f"small.{n}.image"]), (n, SMALL[n])
        assert np.array_equal(out["label"][0].cpu().numpy(), GOLD[f"small.{n}.label"]), (n, SMALL[n])
        assert np.array_equal(next_draws(), GOLD[f"small.{n}.next"]), n
    return store


def check_mixed_batch(store, count, patch, seed):
    """One call for `count` slices of different extents and branches == the same samples one at a time with `params=` given."""
    idx = [(7 * j + 3) % len(store) for j in range(count)]
    seed_both(seed)
    params = [draw_generator(store.images[i].shape, patch) for i in idx]
    assert {p[2] for p in params} == {BRANCH_NONE, BRANCH_ROTFLIP, BRANCH_ROTATE} and len({p[:2] for p in params}) > 3
    seed_both(seed)
    both = OnDeviceAugment2D(store, patch).batch(idx)
    assert both["image"].shape == (count, 1) + tuple(patch) and both["label"].shape == (count,) + tuple(patch)
    for j, i in enumerate(idx):
        one = OnDeviceAugment2D(store, patch).batch([i], params=[params[j]])
        assert torch.equal(both["image"][j], one["image"][0]) and torch.equal(both["label"][j], one["label"][0]), j


def test_fused_generator_kernel_equals_the_reference(emu_library):
    store = check_small_cases("cpu")
    check_mixed_batch(store, 9, (24, 20), 77)
    check_mixed_batch(store, 35, (6, 5), 78)            # more than one launch: 32 samples, then 3


def host_real_case(image, label, patch, seed):
    seed_both(seed)
    s = RandomGenerator(list(patch))({"image": image, "label": label})
    return s["image"].numpy(), s["label"].numpy()


def device_real_case(device):
    def run(image, label, patch, seed):
        store = DeviceSliceStore([(image, label)], device)
        seed_both(seed)
        out = OnDeviceAugment2D(store, patch).batch([0])
        return out["image"][0].cpu().numpy(), out["label"][0].cpu().numpy()
    return run


def check_real_cases(make, cases=None):
    """ACDC extents -> 256 x 256 and 224 x 224 as digests.  ``make(image, label, patch, seed)`` -> (image [1, O0, O1] fp32, label uint8)."""
    for n in (range(len(REAL)) if cases is None else cases):
        n0, n1, o0, o1, seed = REAL[n]
        image, label = case_slice((n0, n1), seed)
        img, lab = make(image, label, (o0, o1), seed)
        assert img.dtype == np.float32 and lab.dtype == np.uint8 and img.shape == (1, o0, o1) and lab.shape == (o0, o1)
        assert_digest(img[None], f"real.{n}.image")
        assert_digest(lab[None, None], f"real.{n}.label")


def test_host_random_generator_at_the_real_extents():
    check_real_cases(host_real_case)


@pytest.mark.slow
def test_fused_kernel_at_a_real_extent(emu_library):
    """512 x 428 -> 224 x 224 (a zero-edge pair) and the first rotate case, through the emulated kernel."""
    rotate = next(n for n, c in enumerate(REAL) if draw_after_seed(c[4]) == BRANCH_ROTATE)
    edge = next(n for n, c in enumerate(REAL) if c[:4] == (512, 428, 224, 224))
    check_real_cases(device_real_case("cpu"), cases=sorted({rotate, edge}))


def check_resize_cases(device):
    """`icl_slice_resize` == scipy's zoom(order=0), fp32 and int64, the zero-edge pairs included (ZOOM_CASES)."""
    assert any(zoom_edge_is_zero(s[0], d[0]) or zoom_edge_is_zero(s[1], d[1]) for _, s, d, _ in ZOOM_CASES)
    for n, (slices, src, dst, seed) in enumerate(ZOOM_CASES):
        for kind, dtype in (("f32", torch.float32), ("i64", torch.int64)):
            x = torch.from_numpy(zoom_input(kind, slices, src, seed)).to(device)
            y = resize_slices(x, dst)
            assert y.dtype == dtype and y.shape == (slices,) + tuple(dst) and y.device == x.device
            if f"zoom.{n}.{kind}" in GOLD:
                assert np.array_equal(y.cpu().numpy(), GOLD[f"zoom.{n}.{kind}"]), (n, kind)
            else:
                assert_digest(y.cpu().numpy()[None], f"zoom.{n}.{kind}")


def test_slice_resize_equals_scipy_zoom(emu_library):
    check_resize_cases("cpu")


@pytest.mark.parametrize("tag", sorted(SAMPLER_CASES))
def test_two_stream_batches_equal_the_2d_reference_stream(tag):
    nlab, ntot, bs, sbs, seed, epochs = SAMPLER_CASES[tag]
    np.random.seed(seed)
    s = TwoStreamBatchSampler(list(range(nlab)), list(range(nlab, ntot)), bs, sbs)
    rows = []
    for _ in range(epochs):
        rows += [list(map(int, b)) for b in s]
    assert np.array_equal(np.array(rows, dtype=np.int64), GOLD[f"sampler.{tag}.batches"])
    assert len(s) == nlab // (bs - sbs)


def test_compat_root_resolves_the_2d_trainers_dataset_import():
    """`PYTHONPATH=compat:<repo>`: line 17 of train_inherent_consistent_unet_2D.py / ..._swinunet_2D.py."""
    code = ("from dataloaders.dataset import BaseDataSets, RandomGenerator, TwoStreamBatchSampler\n"
            "import icl_amd.dataloaders.dataset as d\n"
            "assert BaseDataSets is d.BaseDataSets and RandomGenerator is d.RandomGenerator\n"
            "assert TwoStreamBatchSampler is d.TwoStreamBatchSampler\n"
            "assert BaseDataSets.__module__ == RandomGenerator.__module__ == 'icl_amd.dataloaders.dataset'\n"
            "print('compat ok')\n")
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "compat") + os.pathsep + ROOT, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd="/tmp", timeout=300)
    assert out.returncode == 0 and "compat ok" in out.stdout, out.stdout + out.stderr


def test_base_datasets_reads_the_reference_layout(tmp_path, capsys):
    """The list files, `num` on the training list only, `idx` in every sample, and the refusal of the CTAugment arguments."""
    from icl_amd.dataloaders.dataset import BaseDataSets
    (tmp_path / "train_slices.list").write_text("a_slice_1\na_slice_2\nb_slice_1\n")
    (tmp_path / "val_test.list").write_text("a\nb\n")
    base = str(tmp_path)
    train = BaseDataSets(base_dir=base, split="train", num=2, transform=RandomGenerator([8, 8]))
    val = BaseDataSets(base_dir=base, split="val_test", num=1)
    assert train.sample_list == ["a_slice_1", "a_slice_2"] and val.sample_list == ["a", "b"] and len(train) == 2
    assert "total 2 samples" in capsys.readouterr().out
    image, label = case_slice((10, 12), 1)
    train.read_case = lambda idx: (image, label)
    val.read_case = lambda idx: (image[None], label[None])
    seed_both(4)
    got = train[1]
    seed_both(4)
    want = RandomGenerator([8, 8])({"image": image, "label": label})
    assert got["idx"] == 1 and torch.equal(got["image"], want["image"]) and torch.equal(got["label"], want["label"])
    assert val[0]["idx"] == 0 and val[0]["image"].shape == (1, 10, 12)
    store = DeviceSliceStore.from_dataset(train, "cpu")
    assert len(store) == 2 and store.images[0].dtype == torch.float32 and store.labels[0].dtype == torch.uint8
    with pytest.raises(NotImplementedError, match="CTAugment"):
        BaseDataSets(base_dir=base, split="train", ops_weak=[("x", ())], ops_strong=[("y", ())])


def test_launchers_refuse_bad_arguments_with_a_message(emu_library):
    store = DeviceSliceStore([case_slice((10, 12), 1)], "cpu")
    good = (10, 12, BRANCH_ROTFLIP, 1, 0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 11 / 7, 9 / 7)
    OnDeviceAugment2D(store, (8, 8)).batch([0], params=[good])
    with pytest.raises(RuntimeError, match="batch 0 out of range"):
        _lib.check(_lib.lib().icl_slice_augment(*raw_augment_args(store, good), 0, *raw_outputs(8, 8), 8, 8, None), "slice_augment")
    with pytest.raises(RuntimeError, match="batch 33 out of range"):
        _lib.check(_lib.lib().icl_slice_augment(*raw_augment_args(store, good), 33, *raw_outputs(8, 8), 8, 8, None), "slice_augment")
    with pytest.raises(RuntimeError, match="output extents 1 x 8"):
        OnDeviceAugment2D(store, (1, 8)).batch([0], params=[good])
    with pytest.raises(RuntimeError, match="k = 4 outside 0..3"):
        OnDeviceAugment2D(store, (8, 8)).batch([0], params=[good[:3] + (4,) + good[4:]])
    with pytest.raises(RuntimeError, match="unknown branch 3"):
        OnDeviceAugment2D(store, (8, 8)).batch([0], params=[good[:2] + (3,) + good[3:]])
    with pytest.raises(RuntimeError, match="extents 0 x 12"):
        OnDeviceAugment2D(store, (8, 8)).batch([0], params=[(0,) + good[1:]])
    with pytest.raises(RuntimeError, match="null pointer"):
        _lib.check(_lib.lib().icl_slice_augment(None, None, None, None, 1, None, None, 8, 8, None), "slice_augment")
    x = torch.zeros(2, 10, 12)
    y = torch.zeros(2, 8, 8)
    L = _lib.lib()
    with pytest.raises(RuntimeError, match="batch 0 out of range"):
        _lib.check(L.icl_slice_resize(x.data_ptr(), y.data_ptr(), 0, 10, 12, 8, 8, 0, None), "slice_resize")
    with pytest.raises(RuntimeError, match="output extents 8 x 1"):
        _lib.check(L.icl_slice_resize(x.data_ptr(), y.data_ptr(), 2, 10, 12, 8, 1, 0, None), "slice_resize")
    with pytest.raises(RuntimeError, match="more than 2\\^31 - 1 pixels"):
        _lib.check(L.icl_slice_resize(x.data_ptr(), y.data_ptr(), 2, 10, 12, 1 << 16, 1 << 16, 0, None), "slice_resize")
    with pytest.raises(RuntimeError, match="source extents 0 x 12"):
        _lib.check(L.icl_slice_resize(x.data_ptr(), y.data_ptr(), 2, 0, 12, 8, 8, 0, None), "slice_resize")
    with pytest.raises(RuntimeError, match="unknown element kind 2"):
        _lib.check(L.icl_slice_resize(x.data_ptr(), y.data_ptr(), 2, 10, 12, 8, 8, 2, None), "slice_resize")
    with pytest.raises(RuntimeError, match="null pointer"):
        _lib.check(L.icl_slice_resize(None, y.data_ptr(), 2, 10, 12, 8, 8, 0, None), "slice_resize")
    with pytest.raises(ValueError):
        resize_slices(torch.zeros(2, 10, 12, dtype=torch.float64), (8, 8))


def test_val_resize_switch_refuses_unknown_values(monkeypatch):
    from icl_amd import val_2D
    monkeypatch.setenv("ICL_VAL_RESIZE", "gpu")
    with pytest.raises(ValueError, match="ICL_VAL_RESIZE"):
        val_2D.val_resize_mode()


_KEEP = []


def raw_augment_args(store, rec):
    import ctypes
    ptrs = ctypes.c_void_p * 1
    args = (ptrs(store.images[0].data_ptr()), ptrs(store.labels[0].data_ptr()), (ctypes.c_int32 * 5)(*rec[:5]), (ctypes.c_double * 8)(*rec[5:]))
    _KEEP.append(args)
    return args


def raw_outputs(o0, o1):
    image, label = torch.zeros(1, 1, o0, o1), torch.zeros(1, o0, o1, dtype=torch.uint8)
    _KEEP.append((image, label))
    return image.data_ptr(), label.data_ptr()


def test_device_assembly_keeps_products_and_sums_apart_and_uses_no_scratch(tmp_path):
    """scipy's C code rounds every product and every sum of the rotate / zoom coordinates on its own; hipcc contracts a * b + c into
    an fma unless told otherwise (`fp contract(off)` in datafeed.h).  The device assembly of the new kernels, built with the flags
    of icl_amd/build.py, must hold no fp64 fma and use no scratch memory."""
    from icl_amd.build import FLAGS
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc on this host")
    csrc = os.path.join(ROOT, "icl_amd", "csrc")
    rs = "(const {0}*, {0}*, int, int, int, int, int, double, double)"
    src = tmp_path / "feed2d.hip"
    src.write_text('#include <hip/hip_runtime.h>\n#include <stdint.h>\n#include "device_env_hip.h"\n#include "kernels/common.h"\n'
                   '#include "kernels/datafeed.h"\n'
                   "__global__ void keep_augment(icl::SliceBatch sb, float* a, uint8_t* b) {}\n"
                   "auto* keep = &icl::slice_augment_kernel;\n"
                   f"template __global__ void icl::slice_resize_kernel<float>{rs.format('float')};\n"
                   f"template __global__ void icl::slice_resize_kernel<long long>{rs.format('long long')};\n")
    out = tmp_path / "feed2d.s"
    subprocess.check_call([hipcc, *FLAGS, "-I", csrc, "-S", "--cuda-device-only", "-o", str(out), str(src)], stderr=subprocess.DEVNULL)
    text = out.read_text()
    seen = []
    for m in re.finditer(r"^(_ZN3icl\d+slice_(?:augment|resize)_kernel\w+):[^\n]*\n(.*?)s_endpgm", text, re.S | re.M):
        seen.append(m.group(1))
        body = m.group(2)
        fused = [ln for ln in body.splitlines() if re.search(r"v_fma\w*_f64", ln)]
        assert not fused, (m.group(1), fused[:3])
        assert "v_mul_f64" in body and "v_add_f64" in body, m.group(1)
        assert not re.search(r"\b(scratch_|buffer_(load|store))", body), m.group(1)
        meta = re.search(r"\.amdhsa_kernel " + re.escape(m.group(1)) + r"\n(.*?)\.end_amdhsa_kernel", text, re.S).group(1)
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", meta), m.group(1)
    assert len(seen) == 3, seen
