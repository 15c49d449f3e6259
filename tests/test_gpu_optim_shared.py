"""What icl_amd.optim.FusedSGD and FusedAdamW share (the step scope of the forward pre-hook, ``_icl_factors``, the single-process decision,
the gradient collector and its refusals) on the MI355X: every entry of tests/optim_shared_ref.py's table exactly as
test_optim_shared_emu.py runs it on the emulation."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import optim_shared_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from icl_amd import _lib
    assert _lib.lib_path().endswith("libicl_hip.so"), "GPU tests must run on the HIP library"
    return torch.device("cuda", 0)


@pytest.mark.parametrize("name", list(ref.CHECKS))
def test_optim_shared(dev, name):
    ref.CHECKS[name](dev)
