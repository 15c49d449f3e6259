"""Host logic of the connected-component post-processing (no device): ``keep_components`` on host data against the scipy restatement of
tests/components_ref.py, ``components_mode``, and the ``postprocess=`` keyword of the four validation loops — None leaves every result as
it was, ``"largest"`` removes a planted speck and moves the Dice to the value worked out by hand."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import components_ref as cr  # noqa: E402
from icl_amd import val_2D, val_3D  # noqa: E402
from icl_amd.val_3D import components_mode, keep_components  # noqa: E402


class _RoundNet(torch.nn.Module):
    """logits[:, k] = -(x - k)^2: the arg-max is the input rounded to the nearest class — the prediction is the image."""

    def __init__(self, classes):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.classes = classes

    def forward(self, x, inference=False):
        return torch.cat([-(x - k) ** 2 for k in range(self.classes)], dim=1)


@pytest.mark.parametrize("k", cr.CONNECTIVITIES)
@pytest.mark.parametrize("name", list(cr.CASES))
def test_keep_components_on_host_data(name, k):
    m, nc = cr.CASES[name]()
    for keep_largest, min_size in cr.filter_settings(m, nc, k):
        out = keep_components(m, nc, k, keep_largest, min_size)
        assert isinstance(out, np.ndarray)
        cr.check_filter(m, out, nc, k, keep_largest, min_size)
    t = torch.from_numpy(np.ascontiguousarray(m))
    out = keep_components(t, nc, connectivity=k)
    assert torch.is_tensor(out) and out.dtype == t.dtype and out.device == t.device
    cr.check_filter(m, out.numpy(), nc, k, True, 0)


def test_keep_components_keeps_other_dtypes_and_refuses_bad_arguments():
    m, nc = cr.CASES["random_nc4_d5"]()
    for dt in (np.int16, np.int32, np.float32):
        out = keep_components(m.astype(dt), nc)
        assert out.dtype == dt and np.array_equal(out, cr.keep_reference(m, nc, 1).astype(dt))
    for kw in (dict(connectivity=0), dict(connectivity=4), dict(connectivity=1.0), dict(min_size=-1), dict(min_size=0.5),
               dict(num_classes=1)):
        arg = dict(num_classes=nc)
        arg.update(kw)
        with pytest.raises(ValueError):
            keep_components(m, **arg)
    with pytest.raises(ValueError):
        keep_components(m[0], nc)                       # 2-D
    with pytest.raises(ValueError):
        keep_components(np.stack((m, m)), nc)           # a leading axis longer than 1


def test_components_mode(monkeypatch):
    monkeypatch.delenv("ICL_VAL_COMPONENTS", raising=False)
    assert components_mode() == "device"
    for v in ("device", "host"):
        monkeypatch.setenv("ICL_VAL_COMPONENTS", v)
        assert components_mode() == v
    monkeypatch.setenv("ICL_VAL_COMPONENTS", "scipy")
    with pytest.raises(ValueError):
        components_mode()


def _speck_maps(shape):
    """gt: a block of class 1 and a block of class 2.  pred: the same blocks, class 1 one plane short, plus a one-voxel speck of class 1
    far from it.  By hand, class 1: |G| = 4 * 4 * 4 = 64, |P| = 3 * 4 * 4 + 1 = 49 with the speck, 48 without, |P & G| = 48: Dice
    96 / 113 with the speck and 96 / 112 without; class 2 is untouched (Dice 1)."""
    gt = np.zeros(shape, np.uint8)
    gt[1:5, 2:6, 2:6] = 1
    gt[1:3, 8:10, 7:9] = 2
    pred = gt.astype(np.int64)
    pred[4, 2:6, 2:6] = 0
    speck = (shape[0] - 1, shape[1] - 1, shape[2] - 1)
    assert gt[speck] == 0
    pred[speck] = 1
    return gt, pred, speck


def test_all_case_base_postprocess():
    net = _RoundNet(3)
    gt, pred, speck = _speck_maps((12, 14, 10))
    run = lambda **kw: val_3D.test_all_case_base(net, "unet_3D", None, num_classes=3, patch_size=(12, 14, 10), stride_xy=8, stride_z=8,  # noqa: E731
                                                 cases=[(pred.astype(np.float32), gt)], **kw)
    plain = run()
    assert run(postprocess=None) == plain
    assert [m[0][0] for m in plain] == [96 / 113, 1.0]
    for post in ("largest", {"keep_largest": True}, {"keep_largest": False, "min_size": 2}, {"connectivity": 3}):
        got = run(postprocess=post)
        assert [m[0][0] for m in got] == [96 / 112, 1.0], post
    assert run(postprocess={"keep_largest": False}) == plain          # nothing to drop
    for bad in ("biggest", 3, {"size": 2}, {"connectivity": 0}, {"min_size": -1}):
        with pytest.raises(ValueError):
            run(postprocess=bad)


def test_all_case_amos_postprocess():
    net = _RoundNet(3)
    gt, pred, speck = _speck_maps((12, 14, 10))
    loader = [{"image": torch.from_numpy(pred.astype(np.float32))[None, None], "label": torch.from_numpy(gt.astype(np.int64))[None, None]}]
    run = lambda **kw: val_3D.test_all_case_amos(net, "unet_3D", loader, num_classes=3, **kw)      # noqa: E731
    plain = run()
    assert run(postprocess=None) == plain
    assert [m[0][0] for m in plain] == [96 / 113, 1.0]
    assert [m[0][0] for m in run(postprocess="largest")] == [96 / 112, 1.0]
    with pytest.raises(ValueError):
        run(postprocess="biggest")


@pytest.mark.parametrize("fn", ["test_single_volume", "test_single_volume_ours"])
def test_single_volume_postprocess(fn):
    net = _RoundNet(3)
    gt, pred, speck = _speck_maps((6, 16, 12))
    image = torch.from_numpy(pred.astype(np.float32))[None]
    label = torch.from_numpy(gt)[None]
    run = lambda **kw: getattr(val_2D, fn)(image, label, net, classes=3, patch_size=(16, 12), **kw)      # noqa: E731
    plain = run()
    assert run(postprocess=None) == plain
    assert [m[0] for m in plain] == [96 / 113, 1.0]
    # the stacked [slices, H, W] prediction is ONE 3-D map: the block spans four slices and stays whole
    assert [m[0] for m in run(postprocess="largest")] == [96 / 112, 1.0]
    assert [m[0] for m in run(postprocess={"keep_largest": False, "min_size": 48})] == [96 / 112, 0]      # class 2 has 8 voxels
    assert [m[0] for m in run(postprocess={"keep_largest": False, "min_size": 49})] == [0, 0]      # class 1 vanishes from the prediction too
    with pytest.raises(ValueError):
        run(postprocess="biggest")


def test_compat_modules_re_export_the_new_names():
    import importlib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "compat"))
    try:
        for name in ("val_3D", "val_2D"):
            sys.modules.pop(name, None)
        m3 = importlib.import_module("val_3D")
        assert m3.keep_components is keep_components and m3.components_mode is components_mode
    finally:
        sys.path.remove(os.path.join(root, "compat"))
        for name in ("val_3D", "val_2D"):
            sys.modules.pop(name, None)
