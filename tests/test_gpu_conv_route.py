"""The convolution operators of icl_amd/ops.py on the MI355X make the library calls they made before `ops.plan_conv3d` decided their
route: tests/golden/conv_route_gpu.json was recorded on the parent commit, on this chip and with its library, by
tests/golden/make_golden_conv_route_gpu.py — per case of conv_route_checks.CASES_GPU every library call of forward + backward (entry
point, arguments, stream, return value, kernel) and exact checksums of y and the gradients (fixed summation orders: DESIGN.md §4.4)."""
import json
import os

import pytest
import torch

import conv_route_checks as C

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_route_gpu.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_golden_has_every_case_and_reaches_every_form(golden):
    assert sorted(golden) == sorted(C.case_id(c) for c in C.CASES_GPU)
    seen = set().union(*(C.forms_of(c, golden[C.case_id(c)]["trace"]) for c in C.CASES_GPU))
    assert not [f for f in C.FORMS_GPU if f not in seen]


@pytest.mark.parametrize("c", C.CASES_GPU, ids=C.case_id)
def test_calls_and_bits_are_those_before_the_route(monkeypatch, golden, c):
    got = json.loads(json.dumps(C.run_case(monkeypatch, torch.device("cuda", 0), c)))
    print(json.dumps(got))
    want = golden[C.case_id(c)]
    assert got["trace"] == want["trace"]
    assert got["sums"] == want["sums"]
