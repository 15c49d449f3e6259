"""What icl_amd.optim.FusedSGD and FusedAdamW share (the step scope of the forward pre-hook, ``_icl_factors``, the single-process decision,
the gradient collector and its refusals) on the CPU emulation of the kernel sources: every entry of tests/optim_shared_ref.py's table,
each for both optimisers.  The same table runs on the device in test_gpu_optim_shared.py."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "hipemu"))
from build_emu import build_emu  # noqa: E402
import optim_shared_ref as ref  # noqa: E402

from icl_amd import _lib  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def emu_library():
    _lib._use_library_for_tests(build_emu(), host_pointers=True)
    yield
    _lib._use_library_for_tests(None)


@pytest.mark.parametrize("name", list(ref.CHECKS))
def test_optim_shared(name):
    ref.CHECKS[name]("cpu")
