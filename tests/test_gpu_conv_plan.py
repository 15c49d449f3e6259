"""The forward planner on the MI355X: the launches of every layer shape are those of the commit before it.

tests/golden/conv_plan_gpu.json was recorded on that commit, on this chip, by tests/golden/make_golden_conv_plan_gpu.py from
conv_plan_checks.launch_record: per shape (the layers of tests/test_conv_plan.py at batch 2, real extents — the plan is a function of the
exact extents and of the chip's 256 CUs) the kernel names, slab counts, both numbers of icl_last_wgrad_grid, the live-forward kernel and
an integer checksum of every output.  The checksums match exactly: these kernels sum in fixed orders."""
import json
import os

import pytest
import torch

from conv_plan_checks import FALLBACK_CASES, SHAPES, _fill, check_pointer_fallbacks, launch_record

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_plan_gpu.json")
LAYERS = [sh for sh in SHAPES if sh not in ((20, 24, 24), (16, 16, 20))]      # without the two ragged ones


@pytest.fixture(scope="module")
def pool():
    dev = torch.device("cuda", 0)
    numel = max(2 * max(cin, cout) * e ** 3 for cin, cout, e in LAYERS)
    return {"x": _fill(numel, 1, dev), "gy": _fill(numel, 2, dev)}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_table_has_every_layer(golden):
    assert sorted(golden) == sorted(f"{cin}|{cout}|{e}" for cin, cout, e in LAYERS)


@pytest.mark.parametrize("cin,cout,e", LAYERS)
def test_launches_are_those_before_the_planner(monkeypatch, pool, golden, cin, cout, e):
    for k in [k for k in os.environ if k.startswith(("ICL_CONV_", "ICL_WGRAD_"))]:
        monkeypatch.delenv(k)
    got = launch_record(torch.device("cuda", 0), cin, cout, e, pool)
    print(json.dumps(got))
    assert got == golden[f"{cin}|{cout}|{e}"]


@pytest.mark.parametrize("d,h,w", sorted(FALLBACK_CASES))
def test_split_launch_decides_on_its_pointers(monkeypatch, d, h, w):
    check_pointer_fallbacks(monkeypatch, torch.device("cuda", 0), d, h, w)
