"""The voxel-wise loss kernels (csrc/kernels/loss_point.h: softmax KL, entropy, focal), their launchers, ops.softmax_kl / ops.entropy /
ops.focal_loss and the functions of icl_amd.utils.losses built on them, on the CPU emulation of the kernel sources: every entry of
tests/point_loss_ref.py's table — forward and backward against the fp64 restatements for 2, 3, 16 and 17 classes, the class-walking body
forced at 3 classes, the last-axis soft-max of compute_kl_loss, extreme logits, exact zeros, labels outside the class range, permuted
views, refused arguments — and the tie of those restatements to what the reference's own functions gave
(tests/golden/point_losses.npz).  The same table runs on the device in test_gpu_point_loss.py."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "hipemu"))
from build_emu import build_emu  # noqa: E402
import point_loss_ref as ref  # noqa: E402

from icl_amd import _lib  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def emu_library():
    _lib._use_library_for_tests(build_emu(), host_pointers=True)
    yield
    _lib._use_library_for_tests(None)


@pytest.mark.parametrize("name", list(ref.CHECKS))
def test_point_loss(name):
    ref.CHECKS[name]("cpu")


def test_restatements_reproduce_the_reference_golden():
    ref.check_golden()


def test_trainer_options_default_to_todays_objective():
    """ICLConfig.consistency / w_ent default to "mse" and 0.0 (a wrong string is refused in the table's "refusals" entry)."""
    from icl_amd.trainer import ICLConfig
    cfg = ICLConfig()
    assert cfg.consistency == "mse" and cfg.w_ent == 0.0
