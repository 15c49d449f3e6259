"""The pooling / resize / depth-to-space kernels (csrc/kernels/pool_resize.h) and their launchers' dispatch on the CPU emulation of the
kernel sources: every entry of tests/resample_ref.py's table — parity with fp64 (resize, transposed convolution) or with torch bit for
bit (max-pool, NaN included), and the kernel each case reached.  The same table runs on the device in test_gpu_resample.py."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "hipemu"))
from build_emu import build_emu  # noqa: E402
import resample_ref as ref  # noqa: E402

from icl_amd import _lib  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def emu_library():
    _lib._use_library_for_tests(build_emu(), host_pointers=True)
    yield
    _lib._use_library_for_tests(None)


@pytest.mark.parametrize("name", list(ref.CHECKS))
def test_resample(name):
    ref.CHECKS[name]("cpu")
