"""The gradient-clipping kernels (csrc/kernels/gradclip.h), their launchers, icl_amd.optim.clip_grad_norm_ and the max_grad_norm option of
FusedAdamW / FusedSGD on the CPU emulation of the kernel sources: every entry of tests/gradclip_ref.py's table — the norm of dense and
factored gradients within one fp32 ulp of the fp64 reference (factors multiplied out), coefficient and scaled values bit for bit,
sentinels, refused arguments, both optimisers with a binding clip against the fp64 chain and the torch yardstick, the free function
against the option bit for bit, and the trainer's switch.  The same table runs on the device in test_gpu_gradclip.py."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "hipemu"))
from build_emu import build_emu  # noqa: E402
import gradclip_ref as ref  # noqa: E402

from icl_amd import _lib  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def emu_library():
    _lib._use_library_for_tests(build_emu(), host_pointers=True)
    yield
    _lib._use_library_for_tests(None)


@pytest.mark.parametrize("name", list(ref.CHECKS))
def test_gradclip(name):
    ref.CHECKS[name]("cpu")
