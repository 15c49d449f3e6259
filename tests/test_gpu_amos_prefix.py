"""AMOS cached prefix on the MI355X, through the C ABI (csrc/kernels/prefix.h, icl_prefix_box / icl_prefix_resample / icl_prefix_restore,
icl_amd/dataloaders/amos.py): exactly the literal numpy chain of tests/amos_prefix_ref.py, on the case list of test_amos_prefix_emu.py and
on one mid-size case; the raw-to-batch path against the host-prepared store; the validation items; torch's grid_sample as an independent
implementation.  Parity with MONAI's own code is unpinned (MONAI and nibabel are not installed)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import amos_feed_ref as feed_ref  # noqa: E402
import amos_prefix_ref as ref  # noqa: E402

from icl_amd.dataloaders.amos import (OnDeviceAugmentAMOS, amos_val_cases_from_raw, amos_volume_store,  # noqa: E402
                                      amos_volume_store_from_raw, restore_label)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from icl_amd import _lib
    assert _lib.lib_path().endswith("libicl_hip.so"), "GPU tests must run on the HIP library"
    return torch.device("cuda", 0)


def test_case_list_on_the_gpu_equals_the_literal_chain(dev):
    for case in ref.CASES:
        got_i, _, _ = ref.check_case(case, dev)
        assert got_i.is_cuda


@pytest.mark.parametrize("case", [ref.QUAD_CASE, ref.QUAD_CASE_RESCALED, ref.QUAD_CASE_REVERSED], ids=["identity", "rescaled", "reversed"])
def test_quad_outputs_on_aligned_and_offset_buffers(dev, case):
    got_i, got_l, plan = ref.check_case(case, dev)
    assert plan.out_shape[2] % 4 == 0 and got_i.data_ptr() % 16 == 0 and got_l.data_ptr() % 4 == 0
    ref.check_case(case, dev, out=ref.misaligned_outputs(plan.out_shape, dev))


def test_mid_size_case_runs_many_workgroups_and_repeats_bit_for_bit(dev):
    """Raw (96, 80, 40) at (0.8, 0.8, 5.0): 300 workgroups' partial boxes for the finishing workgroup, an output of (51, 42, 94)."""
    got_i, got_l, plan = ref.check_case(ref.MID_CASE, dev)
    assert plan.box == (1, 1, 1, 95, 79, 39) and plan.out_shape == (51, 42, 94)
    again_i, again_l, again = ref.run_case(ref.MID_CASE, dev)
    assert again == plan and torch.equal(again_i, got_i) and torch.equal(again_l, got_l)
    ref.check_restore(ref.MID_CASE, dev, identity=False)


def test_box_kernel_loops_on_a_volume_larger_than_its_grid(dev):
    """Raw (160, 128, 111): more groups of four voxels than the box kernel's 1,024 workgroups x 256 threads, so its threads loop.  The
    respacing is left alone (spacing = pixdim), so the result is the oriented crop itself."""
    case = ref.make_case((160, 128, 111), "inside", ref.ORIENTATIONS[3], ref.PIXDIM, seed=9)
    assert 160 * 128 * 111 > 4 * 1024 * 256
    _, _, plan = ref.check_case(case, dev)
    assert plan.out_shape == (158, 126, 109)


@pytest.mark.parametrize("index", range(len(ref.TILE_CASES)))
def test_several_tiles_along_oriented_axis_2(dev, index):
    """More outputs along oriented axis 2 than one tile holds (test_amos_prefix_emu.py says what that exercises)."""
    case = ref.TILE_CASES[index]
    _, _, plan = ref.check_case(case, dev)
    assert plan.out_shape[2] > min(512, int(252 / (plan.pixdim[2] / plan.spacing[2])) + 1)
    if plan.out_shape[2] % 4 == 0:
        ref.check_case(case, dev, out=ref.misaligned_outputs(plan.out_shape, dev))
    ref.check_restore(case, dev, identity=False)


def test_more_tiles_than_workgroups_and_more_voxels_than_restore_threads(dev):
    """Raw (1100, 481, 4): 67,100 tiles for the resample grid's 65,536 workgroups and 2,116,400 voxels for the restore grid's 8,192 x 256
    threads: both kernels' outer loops run a second time."""
    case = ref.MANY_TILES_CASE
    _, _, plan = ref.check_case(case, dev)
    assert plan.out_shape[0] * -(-plan.out_shape[1] // 8) > 65536 and int(np.prod(plan.shape)) > 8192 * 256
    ref.check_restore(case, dev, identity=False)


def test_restore_on_the_gpu(dev):
    for i, ori in enumerate(ref.ORIENTATIONS):
        ref.check_restore(ref.make_case(ref.RAWS[0], ref.BOX_KINDS[i % 4], ori, ref.PIXDIM, route=("axcodes", "affine")[i % 2]), dev, identity=True)
    picked = [c for c in ref.CASES if c["spacing"] != ref.PIXDIM][::3] + [c for c in ref.CASES if c["pad_to"]]
    for case in picked:
        ref.check_restore(case, dev, identity=False)


def test_store_from_raw_feeds_the_same_batches_as_the_host_prepared_store(dev):
    """amos_volume_store_from_raw -> OnDeviceAugmentAMOS.batch with fixed parameter rows == amos_volume_store of the restatement's arrays
    -> the same batch."""
    cases = [ref.CASES[1], ref.CASES[20], ref.MID_CASE, ref.CASES[52]]
    raw = []
    for case in cases:
        image, label, how = ref.case_inputs(case)
        raw.append({"image": image[None], "label": label[None].astype(np.float32), **how})      # channel-first, float label: as LoadImaged gives
    raw[1] = (raw[1]["image"], raw[1]["label"], raw[1]["affine"]) if "affine" in raw[1] else raw[1]
    store, plans = amos_volume_store_from_raw(raw, dev)
    want = [ref.reference(case) for case in cases]
    host_store = amos_volume_store([(w[0], w[1]) for w in want], dev)
    assert len(store) == len(host_store) == 4 and [p.out_shape for p in plans] == [w[0].shape for w in want]
    for i in range(4):
        assert store.images[i].is_cuda and torch.equal(store.images[i], host_store.images[i]) and torch.equal(store.labels[i], host_store.labels[i])
    roi = (8, 8, 8)
    rows = [feed_ref.make_row(w[0].shape, roi, tuple(max(n - r, 0) // 2 for n, r in zip(w[0].shape, roi)), flip, k, 1.0, add)
            for w, flip, k, add in zip(want, (0b101, 0b010, 0b111, 0), (1, 2, 3, 0), (0.0, 0.0625, -0.03125, 0.0))]
    got = OnDeviceAugmentAMOS(store, roi).batch([0, 1, 2, 3], params=rows)
    expect = OnDeviceAugmentAMOS(host_store, roi).batch([0, 1, 2, 3], params=rows)
    assert torch.equal(got["image"], expect["image"]) and torch.equal(got["label"], expect["label"])
    for j in range(4):
        chain_i, chain_l = feed_ref.forward_chain(want[j][0], want[j][1], rows[j], roi)
        assert np.array_equal(got["image"][j].cpu().numpy(), chain_i) and np.array_equal(got["label"][j].cpu().numpy(), chain_l)


def test_validation_items_have_what_the_amos_loop_reads(dev):
    """val_3D.test_all_case_amos: ``batch["image"].to(dev)`` is [1, 1, D, H, W] fp32 for the sliding window, ``batch["label"].squeeze(0)``
    a [1, D, H, W] integer map; with pad_to no extent of the padded grid is below it."""
    cases = [ref.make_case(ref.RAWS[1], "inside", ref.ORIENTATIONS[0], (0.8, 0.8, 5.0)), ref.make_case(ref.RAWS[2], "faces", ref.ORIENTATIONS[13], ref.PIXDIM)]
    raw = [dict(zip(("image", "label"), ref.case_inputs(c)[:2]), **ref.case_inputs(c)[2]) for c in cases]
    items, plans = amos_val_cases_from_raw(raw, dev, pad_to=(12, 12, 12))
    assert len(items) == len(plans) == 2
    for item, plan, case in zip(items, plans, cases):
        image, label = item["image"], item["label"]
        assert image.is_cuda and image.dtype == torch.float32 and tuple(image.shape) == (1, 1) + plan.out_shape
        assert label.dtype == torch.uint8 and tuple(label.shape) == (1, 1) + plan.out_shape and tuple(label.squeeze(0).shape) == (1,) + plan.out_shape
        assert min(plan.padded_shape) >= 12
        image_r, label_r = ref.raw_volume(case["raw"], case["kind"], case["seed"])
        want_i, want_l, _ = ref.forward_chain(image_r, label_r, case["perm"], case["sign"], case["spacing"], case["pixdim"], (12, 12, 12))
        assert np.array_equal(image[0, 0].cpu().numpy(), want_i) and np.array_equal(label[0, 0].cpu().numpy(), want_l)
        prediction = torch.argmax(torch.nn.functional.one_hot(label[0].long(), 16).permute(0, 4, 1, 2, 3), dim=1)     # [1, D, H, W] int64
        assert restore_label(prediction, plan).shape == plan.shape
    default = amos_val_cases_from_raw(raw[:1], dev)[1][0]
    assert default.padded_shape == (96, 96, 96)


@pytest.mark.parametrize("index", range(len(ref.TORCH_IMAGE_CASES)))
def test_image_agrees_with_grid_sample(dev, index):
    """Bound 5e-5 (extents up to 48, values in [0, 1]): torch forms its coordinates in fp32, a few ulp at magnitude <= 48 per axis against
    unit slopes.  The expected values come from torch on the CPU."""
    case = ref.TORCH_IMAGE_CASES[index]
    want, _, _ = ref.torch_reference(case)
    got, _, plan = ref.run_case(case, dev)
    assert max(plan.padded_shape) <= 48                                             # the coordinates' magnitude
    got = got.cpu().numpy()
    assert got.min() >= 0.0 and got.max() <= 1.0
    err = float(np.abs(got - want).max())
    print(f"grid_sample image: case {index} out {plan.out_shape} max abs diff {err:.3e}")
    assert err <= 5e-5, err


def test_label_agrees_with_grid_sample_away_from_ties(dev):
    case = ref.TORCH_LABEL_CASE
    _, want, distance = ref.torch_reference(case)
    assert distance > 1e-3                                                          # the precondition of an exact comparison
    _, got, _ = ref.run_case(case, dev)
    assert np.array_equal(got.cpu().numpy(), want)
