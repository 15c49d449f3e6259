"""The pooling / resize / depth-to-space kernels (csrc/kernels/pool_resize.h) and their launchers' dispatch on the MI355X: every entry of
tests/resample_ref.py's table, exactly as test_resample_emu.py runs it on the emulation — parity with fp64 (resize, transposed
convolution) or with torch bit for bit (max-pool, NaN included), and the kernel each case reached."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import resample_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from icl_amd import _lib
    assert _lib.lib_path().endswith("libicl_hip.so"), "GPU tests must run on the HIP library"
    return torch.device("cuda", 0)


@pytest.mark.parametrize("name", list(ref.CHECKS))
def test_resample(dev, name):
    ref.CHECKS[name](dev)
