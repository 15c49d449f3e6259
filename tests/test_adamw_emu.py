"""The AdamW kernels (csrc/kernels/adamw.h), their launchers and icl_amd.optim.FusedAdamW on the CPU emulation of the kernel sources:
every entry of tests/adamw_ref.py's table — the three kernels against the rule in fp64 inside 4 x torch.optim.AdamW's own error, the
scalars in device memory bit for bit, refused arguments, the optimiser against torch.optim.AdamW with dense, factored and multiplied-out
gradients, state dicts in both directions, the hyper_dev protocol and the trainer's switch.  The same table runs on the device in
test_gpu_adamw.py."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "hipemu"))
from build_emu import build_emu  # noqa: E402
import adamw_ref as ref  # noqa: E402

from icl_amd import _lib  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def emu_library():
    _lib._use_library_for_tests(build_emu(), host_pointers=True)
    yield
    _lib._use_library_for_tests(None)


@pytest.mark.parametrize("name", list(ref.CHECKS))
def test_adamw(name):
    ref.CHECKS[name]("cpu")
