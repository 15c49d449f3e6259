"""Host side of the AMOS cached prefix (icl_amd/dataloaders/amos.py: orientation_from_affine, orientation_from_axcodes, plan_prefix): pure
numpy, no library, no device.  The orientation tables are known by construction (tests/amos_prefix_ref.py builds the affines from them)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import amos_prefix_ref as ref  # noqa: E402

from icl_amd.dataloaders.amos import (PrefixPlan, orientation_from_affine, orientation_from_axcodes, plan_prefix,  # noqa: E402
                                      prefix_out_extent)

SCALES = (0.7, 1.3, 5.0)


@pytest.mark.parametrize("tilt", [0.0, 10.0, -10.0])
def test_all_48_signed_permutations_with_unequal_scales(tilt):
    """Straight, and tilted by 10 degrees about (1, 1, 1): the same table; the zooms are the column norms either way."""
    for perm, sign in ref.ORIENTATIONS:
        got_perm, got_sign, zooms = orientation_from_affine(ref.affine_of(perm, sign, SCALES, tilt_degrees=tilt))
        assert got_perm == perm and got_sign == sign, (perm, sign, tilt)
        assert np.allclose(zooms, ref.source_spacing(perm, SCALES), rtol=1e-14, atol=0), (perm, sign, tilt)
        if tilt == 0.0:
            assert zooms == ref.source_spacing(perm, SCALES)
    assert orientation_from_affine(np.diag([2.0, 3.0, 4.0])) == ((0, 1, 2), (1, 1, 1), (2.0, 3.0, 4.0))          # 3x3 is taken too


def test_axcodes_agree_with_the_affine_route():
    for perm, sign in ref.ORIENTATIONS:
        codes = ref.axcodes_of(perm, sign)
        assert orientation_from_axcodes(codes) == (perm, sign) == orientation_from_affine(ref.affine_of(perm, sign, SCALES))[:2]
        assert orientation_from_axcodes(tuple(codes.lower())) == (perm, sign)
        by_affine = plan_prefix((7, 5, 9), (1, 0, 2, 6, 5, 9), affine=ref.affine_of(perm, sign, SCALES))
        by_codes = plan_prefix((7, 5, 9), (1, 0, 2, 6, 5, 9), spacing=ref.source_spacing(perm, SCALES), axcodes=codes)
        assert by_affine == by_codes and hash(by_affine) == hash(by_codes)
    assert orientation_from_axcodes("LPS") == ((0, 1, 2), (-1, -1, 1)) and orientation_from_axcodes("RAS") == ((0, 1, 2), (1, 1, 1))
    assert orientation_from_axcodes("SRA") == ((1, 2, 0), (1, 1, 1))      # source axis 0 runs up: RAS axis 2 is source axis 0


def test_plan_fields_and_output_extents_follow_the_formula():
    plan = plan_prefix((7, 5, 9), (1, 0, 2, 6, 5, 9), spacing=(0.8, 5.0, 0.8), axcodes="LSP")
    assert isinstance(plan, PrefixPlan) and plan.shape == (7, 5, 9) and plan.box == (1, 0, 2, 6, 5, 9)
    assert plan.perm == (0, 2, 1) and plan.sign == (-1, -1, 1) and plan.spacing == (0.8, 0.8, 5.0) and plan.pixdim == (1.5, 1.5, 2.0)
    assert plan.crop_shape == (5, 7, 5) and plan.pad_front == (0, 0, 0) and plan.padded_shape == (5, 7, 5)
    # rint(4 * 0.8 / 1.5 + 1) = rint(3.13), rint(6 * 0.5333 + 1) = rint(4.2), rint(4 * 2.5 + 1)
    assert plan.out_shape == (3, 4, 11)
    assert plan.window == (-175.0, 425.0, 0.0, 1.0, 1.0) and plan.clip is True
    assert list(plan.int_params()) == [7, 5, 9, 1, 0, 2, 6, 5, 9, 0, 2, 1, -1, -1, 1, 0, 0, 0, 5, 7, 5, 3, 4, 11]
    assert list(plan.double_params()) == [0.8, 0.8, 5.0, 1.5, 1.5, 2.0]
    with pytest.raises(Exception):
        plan.box = (0, 0, 0, 1, 1, 1)                                     # frozen
    for m, s, p in ((9, 0.8, 1.5), (40, 0.78, 1.5), (120, 5.0, 2.0), (1, 3.0, 1.5), (512, 0.78125, 1.5)):
        want = int(np.rint((m - 1) * (np.float64(s) / np.float64(p)) + 1.0))
        assert prefix_out_extent(m, s, p) == ref.out_extent(m, s, p) == want
    # .5 exactly: half to even, down as well as up
    assert prefix_out_extent(6, 3.0, 2.0) == 8          # 5 * 1.5 + 1 = 8.5 -> 8
    assert prefix_out_extent(8, 3.0, 2.0) == 12         # 7 * 1.5 + 1 = 11.5 -> 12
    assert prefix_out_extent(4, 0.75, 1.5) == 2         # 3 * 0.5 + 1 = 2.5 -> 2
    assert plan_prefix((6, 6, 8), (0, 0, 0, 6, 6, 8), spacing=(3.0, 3.0, 3.0), axcodes="RAS", pixdim=(2.0, 2.0, 2.0)).out_shape == (8, 8, 12)
    # the window constants: differences in double, then fp32
    plan = plan_prefix((2, 2, 2), (0, 0, 0, 1, 1, 1), spacing=(1, 1, 1), axcodes="RAS", window=(-0.1, 0.2, 0.1, 0.4, False))
    assert plan.clip is False
    assert plan.window == tuple(float(np.float32(v)) for v in (-0.1, 0.2 - -0.1, 0.1, 0.4 - 0.1, 0.4))


def test_pad_to_arithmetic():
    """w = max(pad_to - extent, 0) per ORIENTED axis, w // 2 in front; the output extent comes from the padded extent."""
    plan = plan_prefix((12, 11, 4), (1, 1, 1, 6, 7, 4), spacing=(1.5, 2.0, 1.5), axcodes="RSA", pad_to=(10, 10, 10))
    assert plan.perm == (0, 2, 1) and plan.crop_shape == (5, 3, 6)
    assert plan.pad_front == (2, 3, 2) and plan.padded_shape == (10, 10, 10) and plan.out_shape == (10, 10, 10)
    plan = plan_prefix((12, 11, 4), (0, 0, 0, 12, 11, 4), spacing=(0.8, 0.8, 5.0), axcodes="RAS", pad_to=(10, 12, 9))
    assert plan.pad_front == (0, 0, 2) and plan.padded_shape == (12, 12, 9)        # widths 0, 1 (0 in front), 5 (2 in front)
    assert plan.out_shape == tuple(ref.out_extent(m, s, 1.5 if a < 2 else 2.0) for a, (m, s) in enumerate(zip((12, 12, 9), (0.8, 0.8, 5.0))))
    assert ref.pad_widths((5, 3, 6), (10, 10, 10)) == [(2, 3), (3, 4), (2, 2)]
    assert plan_prefix((12, 11, 4), (0, 0, 0, 12, 11, 4), spacing=(1, 1, 1), axcodes="RAS", pad_to=None).pad_front == (0, 0, 0)


def test_every_value_error_path():
    ok = dict(spacing=(1.0, 1.0, 1.0), axcodes="RAS")
    with pytest.raises(ValueError, match="empty foreground"):
        plan_prefix((4, 4, 4), (2147483647, 2147483647, 2147483647, 0, 0, 0), **ok)          # what the box kernel leaves without foreground
    with pytest.raises(ValueError, match="empty foreground"):
        plan_prefix((4, 4, 4), (1, 1, 1, 3, 1, 3), **ok)
    with pytest.raises(ValueError, match="outside the volume"):
        plan_prefix((4, 4, 4), (0, 0, 0, 4, 5, 4), **ok)
    with pytest.raises(ValueError, match="outside the volume"):
        plan_prefix((4, 4, 4), (-1, 0, 0, 4, 4, 4), **ok)
    with pytest.raises(ValueError, match="zero column"):
        orientation_from_affine(np.diag([1.0, 0.0, 1.0, 1.0]))
    with pytest.raises(ValueError, match="zero column"):
        plan_prefix((4, 4, 4), (0, 0, 0, 4, 4, 4), affine=np.diag([1.0, 1.0, 0.0, 1.0]))
    with pytest.raises(ValueError, match="4x4"):
        orientation_from_affine(np.eye(2))
    with pytest.raises(ValueError, match="4x4"):
        orientation_from_affine(np.full((4, 4), np.nan))
    for codes in ("RA", "RASS", "RAX", "RLS", "AAS", ("R", "A", 1)):
        with pytest.raises(ValueError, match="orientation_from_axcodes"):
            plan_prefix((4, 4, 4), (0, 0, 0, 4, 4, 4), spacing=(1, 1, 1), axcodes=codes)
    for spacing in ((1.0, 0.0, 1.0), (1.0, -2.0, 1.0), (1.0, np.nan, 1.0), (np.inf, 1.0, 1.0), (1.0, 1.0)):
        with pytest.raises(ValueError, match="spacing"):
            plan_prefix((4, 4, 4), (0, 0, 0, 4, 4, 4), spacing=spacing, axcodes="RAS")
    for pixdim in ((1.5, 0.0, 2.0), (1.5, 1.5), (1.5, np.nan, 2.0)):
        with pytest.raises(ValueError, match="pixdim"):
            plan_prefix((4, 4, 4), (0, 0, 0, 4, 4, 4), pixdim=pixdim, **ok)
    with pytest.raises(ValueError, match="either affine"):
        plan_prefix((4, 4, 4), (0, 0, 0, 4, 4, 4))
    with pytest.raises(ValueError, match="either affine"):
        plan_prefix((4, 4, 4), (0, 0, 0, 4, 4, 4), affine=np.eye(4), axcodes="RAS")
    with pytest.raises(ValueError, match="go together"):
        plan_prefix((4, 4, 4), (0, 0, 0, 4, 4, 4), spacing=(1, 1, 1))
    with pytest.raises(ValueError, match="shape"):
        plan_prefix((4, 4), (0, 0, 0, 4, 4, 4), **ok)
    with pytest.raises(ValueError, match="shape"):
        plan_prefix((65536, 1, 1), (0, 0, 0, 1, 1, 1), **ok)
    with pytest.raises(ValueError, match="pad_to"):
        plan_prefix((4, 4, 4), (0, 0, 0, 4, 4, 4), pad_to=(96, 96), **ok)
    with pytest.raises(ValueError, match="window"):
        plan_prefix((4, 4, 4), (0, 0, 0, 4, 4, 4), window=(1.0, 1.0, 0.0, 1.0, True), **ok)
    with pytest.raises(ValueError, match="output extents"):
        plan_prefix((4, 4, 60000), (0, 0, 0, 4, 4, 60000), spacing=(1.0, 1.0, 5.0), axcodes="RAS")


def test_host_memory_never_reaches_a_launch():
    """Without the tests' emulation library a host array or CPU tensor is refused before the library is even loaded."""
    import torch
    from icl_amd import _lib
    from icl_amd.dataloaders.amos import amos_prefix, restore_label
    assert not _lib.host_pointers_ok()
    image, label = ref.raw_volume((7, 5, 9), "inside")
    with pytest.raises(ValueError, match="amos_prefix: the data must be on a HIP device"):
        amos_prefix(image, label, "cpu", spacing=(1, 1, 1), axcodes="RAS")
    plan = plan_prefix((7, 5, 9), (1, 1, 1, 6, 4, 8), spacing=(1.5, 1.5, 2.0), axcodes="RAS")
    for prediction in (np.zeros(plan.out_shape, dtype=np.uint8), torch.zeros(plan.out_shape, dtype=torch.int64)):
        with pytest.raises(ValueError, match="restore_label: the data must be on a HIP device"):
            restore_label(prediction, plan)


def test_the_yardsticks_own_pieces():
    """The restatement's window, box and inverse on values small enough to state by hand."""
    w = ref.window_volume(np.array([-175.0, 250.0, 37.5, -1000.0, 3000.0], dtype=np.float32))
    assert w.tolist() == [0.0, 1.0, 0.5, 0.0, 1.0]
    image, label = ref.raw_volume((7, 5, 9), "inside")
    assert ref.foreground_box(ref.window_volume(image)) == ((1, 1, 1), (6, 4, 8))
    with pytest.raises(ValueError):
        ref.foreground_box(np.zeros((2, 2, 2), dtype=np.float32))
    out_i, out_l, stages = ref.forward_chain(image, label, (2, 0, 1), (1, -1, 1), (1.5, 1.5, 2.0))
    assert out_i.shape == (7, 5, 3) and np.array_equal(out_l, np.flip(np.transpose(label[1:6, 1:4, 1:8], (2, 0, 1)), 1))
    back = ref.inverse_chain(out_l, (7, 5, 9), stages["box"], (2, 0, 1), (1, -1, 1), (1.5, 1.5, 2.0), (1.5, 1.5, 2.0), stages["widths"])
    assert np.array_equal(back[1:6, 1:4, 1:8], label[1:6, 1:4, 1:8]) and back.sum() == label[1:6, 1:4, 1:8].sum()
