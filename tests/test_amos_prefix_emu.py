"""AMOS cached prefix (csrc/kernels/prefix.h, icl_prefix_box / icl_prefix_resample / icl_prefix_restore, icl_amd/dataloaders/amos.py) on
the CPU emulation of the kernel sources, against the literal numpy chain of tests/amos_prefix_ref.py; the GPU run is in
test_gpu_amos_prefix.py.  Every comparison against the restatement is exact.  Parity with MONAI's own code is unpinned (MONAI and nibabel
are not installed): what is pinned is the definition in DESIGN.md "AMOS cached prefix"."""
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
import amos_prefix_ref as ref  # noqa: E402

from icl_amd import _lib  # noqa: E402
from icl_amd.dataloaders.amos import PREFIX_BOX_WS_INTS, amos_prefix, plan_prefix  # noqa: E402

CPU = torch.device("cpu")


@pytest.fixture(scope="module", autouse=True)
def emu_library():
    _lib._use_library_for_tests(build_emu(), host_pointers=True)
    yield
    _lib._use_library_for_tests(None)


def test_case_list_covers_what_it_claims():
    on_first = [c for c in ref.CASES if c["raw"] == ref.RAWS[0] and c["pad_to"] is None and c["kind"] in ("inside", "faces", "voxel")]
    assert {(c["perm"], c["sign"]) for c in on_first} == set(ref.ORIENTATIONS)
    for raw in ref.RAWS:
        mine = [c for c in ref.CASES if c["raw"] == raw]
        assert {c["kind"] for c in mine} >= {"inside", "faces", "voxel", "flat"} and {c["spacing"] for c in mine} == set(ref.SPACINGS)
    assert any(c["pad_to"] for c in ref.CASES) and {c["route"] for c in ref.CASES} == {"affine", "axcodes"}


@pytest.mark.parametrize("chunk", range(6))
def test_case_list_equals_the_literal_chain(chunk):
    """All 48 orientations on (7, 5, 9), a handful on (12, 11, 4) and (9, 9, 8); boxes inside, on every face, of one voxel, of extent 1 on
    one axis; down-, up- and no respacing; SpatialPad to (10, 10, 10)."""
    mine = ref.CASES[chunk::6]
    assert mine
    for case in mine:
        ref.check_case(case, CPU)


def test_equal_spacing_returns_the_oriented_crop_itself():
    seen = 0
    for case in ref.CASES:
        if case["spacing"] == ref.PIXDIM and case["pad_to"] is None:
            want_i, want_l, stages = ref.reference(case)
            assert np.array_equal(want_i, stages["oriented"][0]) and np.array_equal(want_l, stages["oriented"][1])     # the yardstick itself
            got_i, got_l, _ = ref.run_case(case, CPU)
            assert np.array_equal(got_i.numpy(), stages["oriented"][0]) and np.array_equal(got_l.numpy(), stages["oriented"][1])
            seen += 1
    assert seen >= 16


@pytest.mark.parametrize("case", [ref.QUAD_CASE, ref.QUAD_CASE_RESCALED, ref.QUAD_CASE_REVERSED], ids=["identity", "rescaled", "reversed"])
def test_quad_outputs_on_aligned_and_offset_buffers(case):
    """o2 % 4 == 0: four outputs a thread with one 16-byte and one 4-byte store on aligned buffers; buffers 4 bytes (image) and 1 byte
    (label) off take the one-voxel kernel.  Same result."""
    got_i, got_l, plan = ref.check_case(case, CPU)
    assert plan.out_shape[2] % 4 == 0 and got_i.data_ptr() % 16 == 0 and got_l.data_ptr() % 4 == 0
    ref.check_case(case, CPU, out=ref.misaligned_outputs(plan.out_shape, CPU))
    image, _ = ref.misaligned_outputs(plan.out_shape, CPU)                        # only the image off: still the one-voxel kernel
    ref.check_case(case, CPU, out=(image, torch.empty(plan.out_shape, dtype=torch.uint8)))


@pytest.mark.parametrize("index", range(len(ref.TILE_CASES)))
def test_several_tiles_along_oriented_axis_2(index):
    """More outputs along oriented axis 2 than one tile holds: the tile's first slot is not 0, the launcher's choice of the tile length
    (512, or what 256 slots allow, a multiple of 4 on the quad path) and the span arithmetic decide which voxels are read."""
    case = ref.TILE_CASES[index]
    _, _, plan = ref.check_case(case, CPU)
    ratio = plan.pixdim[2] / plan.spacing[2]
    tile2 = min(512, int(252 / ratio) + 1)                                         # the launcher's rule, restated
    assert plan.out_shape[2] > tile2, (plan.out_shape, tile2)
    if plan.out_shape[2] % 4 == 0:
        ref.check_case(case, CPU, out=ref.misaligned_outputs(plan.out_shape, CPU))  # the same tiles, one output a thread
    ref.check_restore(case, CPU, identity=False)


def test_more_tiles_than_workgroups_and_more_voxels_than_restore_threads():
    case = ref.MANY_TILES_CASE
    _, _, plan = ref.check_case(case, CPU)
    assert plan.out_shape[0] * -(-plan.out_shape[1] // 8) > 65536 and int(np.prod(plan.shape)) > 8192 * 256
    ref.check_restore(case, CPU, identity=False)


def test_an_output_that_is_no_multiple_of_four_is_in_the_list():
    assert any(ref.reference(c)[0].shape[2] % 4 for c in ref.CASES)


def test_label_ties_round_half_to_even():
    """Spacing 3.0 -> 1.5 puts every second coordinate of axis 0 on a half-integer: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2."""
    case = next(c for c in ref.CASES if c["spacing"] == ref.SPACINGS[1] and c["kind"] == "faces" and c["raw"] == ref.RAWS[1])
    _, _, stages = ref.reference(case)
    x, nearest = stages["taps"][0][0], stages["taps"][0][5]
    assert (x[1::2] % 1.0 == 0.5).all() and len(x) > 5 and list(nearest[:6]) == [0, 0, 1, 2, 2, 2]
    ref.check_case(case, CPU)


def test_out_tensors_are_checked():
    case = ref.QUAD_CASE
    _, _, plan = ref.run_case(case, CPU)
    good_i, good_l = torch.empty(plan.out_shape), torch.empty(plan.out_shape, dtype=torch.uint8)
    for bad in ((torch.empty(plan.out_shape, dtype=torch.float64), good_l), (good_i, torch.empty(plan.out_shape, dtype=torch.int64)),
                (torch.empty((1,) + plan.out_shape), good_l), (good_i.to("meta"), good_l),
                (torch.empty(plan.out_shape[0], plan.out_shape[2], plan.out_shape[1]).transpose(1, 2), good_l)):
        with pytest.raises(ValueError, match="out (image|label) must be"):
            ref.run_case(case, CPU, out=bad)


def test_no_foreground_is_a_value_error():
    image = np.full((4, 5, 6), -400.0, dtype=np.float32)
    with pytest.raises(ValueError, match="empty foreground"):
        amos_prefix(image, np.zeros((4, 5, 6), dtype=np.uint8), CPU, spacing=(1, 1, 1), axcodes="RAS")
    image[2, 3, 4] = np.nan                                                       # NaN > 0 is false
    with pytest.raises(ValueError, match="empty foreground"):
        amos_prefix(image, np.zeros((4, 5, 6), dtype=np.uint8), CPU, spacing=(1, 1, 1), axcodes="RAS")


def test_box_on_a_misaligned_image_and_more_than_one_workgroup():
    """The box kernel's scalar path (image 4 bytes off a 16-byte boundary) and its vector path agree; (40, 33, 21) is 27 workgroups'
    partial boxes for the finishing workgroup."""
    image, _ = ref.raw_volume((40, 33, 21), "inside", 3)
    want = ref.foreground_box(ref.window_volume(image))
    consts = plan_prefix((1, 1, 1), (0, 0, 0, 1, 1, 1), spacing=(1, 1, 1), axcodes="RAS").window
    L = _lib.lib()
    buf = torch.zeros(image.size + 8)
    for off in (0, 1):
        shift = off + (-(buf.data_ptr() // 4)) % 4
        view = buf[shift:shift + image.size]
        view.copy_(torch.from_numpy(image.ravel()))
        assert view.data_ptr() % 16 == 4 * off
        box, ws = torch.full((6,), -7, dtype=torch.int32), torch.empty(PREFIX_BOX_WS_INTS, dtype=torch.int32)
        _lib.check(L.icl_prefix_box(view.data_ptr(), *image.shape, (ctypes.c_float * 5)(*consts), 1, box.data_ptr(), ws.data_ptr(), None))
        assert tuple(box[:3].tolist()) == want[0] and tuple(v + 1 for v in box[3:].tolist()) == want[1]


@pytest.mark.parametrize("half", range(2))
def test_restore_with_equal_spacing_returns_the_raw_label_inside_the_box(half):
    for i, ori in enumerate(ref.ORIENTATIONS[half::2]):
        ref.check_restore(ref.make_case(ref.RAWS[0], ref.BOX_KINDS[i % 4], ori, ref.PIXDIM, route=("axcodes", "affine")[i % 2]), CPU, identity=True)


def test_restore_with_a_rescale_equals_the_inverse_chain():
    picked = [c for c in ref.CASES if c["spacing"] != ref.PIXDIM][::3] + [c for c in ref.CASES if c["pad_to"]]
    assert len(picked) >= 12 and {c["raw"] for c in picked} == set(ref.RAWS)
    for case in picked:
        ref.check_restore(case, CPU, identity=False)


# ---- the independent implementation: torch's grid_sample ----------------------------------------------------------------------------------

@pytest.mark.parametrize("index", range(len(ref.TORCH_IMAGE_CASES)))
def test_image_agrees_with_grid_sample(index):
    """Bound 5e-5 (extents up to 48, values in [0, 1]): torch forms its coordinates in fp32, a few ulp at magnitude <= 48 per axis against
    unit slopes."""
    case = ref.TORCH_IMAGE_CASES[index]
    want, _, _ = ref.torch_reference(case)
    got, _, plan = ref.run_case(case, CPU)
    assert max(plan.padded_shape) <= 48                                             # the coordinates' magnitude
    got = got.numpy()
    assert got.min() >= 0.0 and got.max() <= 1.0
    err = float(np.abs(got - want).max())
    print(f"grid_sample image: case {index} out {plan.out_shape} max abs diff {err:.3e}")
    assert err <= 5e-5, err


def test_label_agrees_with_grid_sample_away_from_ties():
    case = ref.TORCH_LABEL_CASE
    _, want, distance = ref.torch_reference(case)
    print(f"grid_sample label: smallest distance to a half-integer {distance:.4f}")
    assert distance > 1e-3                                                          # the precondition of an exact comparison
    _, got, _ = ref.run_case(case, CPU)
    assert np.array_equal(got.numpy(), want)


# ---- the launchers' refusals --------------------------------------------------------------------------------------------------------------

def _plan_arrays(plan, **edits):
    ints = list(plan.int_params())
    doubles = list(plan.double_params())
    for key, value in edits.items():
        kind, pos = key[0], int(key[1:])
        if kind == "i":
            ints[pos] = value
        else:
            doubles[pos] = value
    return (ctypes.c_int32 * 24)(*ints), (ctypes.c_double * 6)(*doubles)


def test_launchers_refuse_bad_arguments_and_write_nothing():
    image, label = ref.raw_volume(ref.RAWS[0], "inside", 0)
    plan = plan_prefix(ref.RAWS[0], (1, 1, 1, 6, 4, 8), spacing=(0.8, 0.8, 5.0), axcodes="LPS")
    L = _lib.lib()
    ti, tl = torch.from_numpy(image.copy()), torch.from_numpy(label.copy())
    oi, ol = torch.full(plan.out_shape, -7.0), torch.full(plan.out_shape, 7, dtype=torch.uint8)
    back = torch.full(plan.shape, 7, dtype=torch.uint8)
    window = plan.window_params()

    def resample(ints, doubles, null=None):
        args = {"image": ti.data_ptr(), "label": tl.data_ptr(), "ints": ints, "doubles": doubles, "window": window, "oi": oi.data_ptr(),
                "ol": ol.data_ptr()}
        if null:
            args[null] = None
        return L.icl_prefix_resample(args["image"], args["label"], args["ints"], args["doubles"], args["window"], 1, args["oi"], args["ol"], None)

    def restore(ints, doubles, kind=0, null=None):
        args = {"pred": ol.data_ptr(), "ints": ints, "doubles": doubles, "out": back.data_ptr()}
        if null:
            args[null] = None
        return L.icl_prefix_restore(args["pred"], kind, args["ints"], args["doubles"], args["out"], None)

    def refused(rc, name, match):
        assert rc == -1
        message = L.icl_last_error().decode()
        assert name in message and match in message, message
        with pytest.raises(RuntimeError, match=name):
            _lib.check(rc, name)
        assert (oi == -7).all() and (ol == 7).all() and (back == 7).all()

    good = _plan_arrays(plan)
    for key in ("image", "label", "ints", "doubles", "window", "oi", "ol"):
        refused(resample(*good, null=key), "prefix_resample", "null pointer")
    for key in ("pred", "ints", "doubles", "out"):
        refused(restore(*good, null=key), "prefix_restore", "null pointer")
    refused(restore(*good, kind=2), "prefix_restore", "unknown element kind 2")
    bad_plans = [({"i0": 0}, "raw extents"), ({"i1": 65536}, "raw extents"), ({"i0": 65535, "i1": 65535, "i2": 2}, "2^31 - 1 voxels"),
                 ({"i9": 1}, "not a permutation"), ({"i10": 3}, "not a permutation"), ({"i12": 0}, "sign 0"),
                 ({"d0": float("nan")}, "finite and positive"), ({"d4": 0.0}, "finite and positive"), ({"d2": float("inf")}, "finite and positive"),
                 ({"d5": -2.0}, "finite and positive"),
                 ({"i3": -1}, "box [-1, 6)"), ({"i7": 6}, "box [1, 6) of raw axis 1 outside the extent 5"), ({"i8": 1}, "box [1, 1)"),
                 ({"i15": -1}, "pad front -1"), ({"i18": 4}, "outside the padded extent 4"),
                 ({"i21": plan.out_shape[0] + 1}, "output extent"), ({"i23": plan.out_shape[2] - 1}, "output extent")]
    for edits, match in bad_plans:
        refused(resample(*_plan_arrays(plan, **edits)), "prefix_resample", match)
        refused(restore(*_plan_arrays(plan, **edits)), "prefix_restore", match)
    assert resample(*good) == 0 and not (oi == -7).any()
    assert restore(*good) == 0
    oi.fill_(-7.0), ol.fill_(7), back.fill_(7)

    box, ws = torch.full((6,), -7, dtype=torch.int32), torch.empty(PREFIX_BOX_WS_INTS, dtype=torch.int32)

    def find_box(n=plan.shape, **null):
        args = {"image": ti.data_ptr(), "window": window, "box": box.data_ptr(), "ws": ws.data_ptr()}
        args.update(null)
        return L.icl_prefix_box(args["image"], *n, args["window"], 1, args["box"], args["ws"], None)

    def box_refused(rc, match):
        refused(rc, "prefix_box", match)
        assert (box == -7).all()

    for key in ("image", "window", "box", "ws"):
        box_refused(find_box(**{key: None}), "null pointer")
    box_refused(find_box((7, 0, 9)), "extents 7 x 0 x 9")
    box_refused(find_box((65536, 1, 1)), "each must be in 1..65535")
    box_refused(find_box((65535, 65535, 2)), "2^31 - 1 voxels")
    box_refused(find_box(window=(ctypes.c_float * 5)(-175.0, 0.0, 0.0, 1.0, 1.0)), "a_max - a_min is 0")
    box_refused(find_box(window=(ctypes.c_float * 5)(-175.0, float("nan"), 0.0, 1.0, 1.0)), "not finite")
    assert find_box() == 0 and box.tolist() == [1, 1, 1, 5, 3, 7]
