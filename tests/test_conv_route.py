"""The convolution operators of icl_amd/ops.py make the library calls they made before `ops.plan_conv3d` decided their route, on the
emulation build: tests/golden/conv_route.json (recorded on the parent commit by tests/golden/make_golden_conv_route.py) holds, per case
of conv_route_checks.CASES_EMU, every library call of forward + backward with its arguments, return value and kernel, and exact
checksums of y and the gradients.  Its "rng" row: the state of torch's CPU generator after each stochastic operator called without a seed."""
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hipemu"))

import conv_route_checks as C  # noqa: E402
from icl_amd import _lib  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_route.json")


@pytest.fixture(scope="module", autouse=True)
def emu_library():
    from build_emu import build_emu
    _lib._use_library_for_tests(build_emu(), host_pointers=True)
    yield
    _lib._use_library_for_tests(None)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_golden_has_every_case_and_reaches_every_form(golden):
    assert sorted(golden) == sorted([C.case_id(c) for c in C.CASES_EMU] + ["rng"])
    seen = set().union(*(C.forms_of(c, golden[C.case_id(c)]["trace"]) for c in C.CASES_EMU))
    assert not [f for f in C.FORMS_EMU if f not in seen]


@pytest.mark.parametrize("c", C.CASES_EMU, ids=C.case_id)
def test_calls_and_bits_are_those_before_the_route(monkeypatch, golden, c):
    got = json.loads(json.dumps(C.run_case(monkeypatch, torch.device("cpu"), c)))
    want = golden[C.case_id(c)]
    assert got["trace"] == want["trace"]
    assert got["sums"] == want["sums"]


def test_stochastic_operators_draw_from_the_cpu_generator_as_before(golden):
    assert C.rng_states(torch.device("cpu")) == golden["rng"]
