"""The forward convolution planner answers the host-only queries exactly as the launcher's dry runs did before it existed.

tests/golden/conv_plan.json holds, per (setting, batch, shape), what the five queries returned on the commit before the planner
(recorded from that commit's emulation build by tests/golden/make_golden_conv_plan.py, which evaluates `table` below): workspace bytes
of the forward (3^3 and 1^3) and of the pre-split forward, the statistics slots, the weight gradient's workspace bytes and the
live-batch answer for every 1 <= n_live <= n.  The planner is host code only, so the emulation build answers as the product does.
"""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hipemu"))

from conv_plan_checks import SHAPES  # noqa: E402
from icl_amd import _lib  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_plan.json")
SWITCHES = ("ICL_CONV_SPLIT", "ICL_CONV_SPLIT_MIN", "ICL_CONV_SPLIT_FLAT", "ICL_CONV_SPLIT_FLAT12", "ICL_CONV_SPLIT_FLAT6",
            "ICL_CONV_SPLIT_KSPLIT", "ICL_CONV_SPLIT_KSPLIT_CUS", "ICL_CONV_FORCE_TILE")
SETTINGS = {
    "default": {},
    "split0": {"ICL_CONV_SPLIT": "0"},
    "ksplit0": {"ICL_CONV_SPLIT_KSPLIT": "0"},
    "cus128": {"ICL_CONV_SPLIT_KSPLIT_CUS": "128"},
    "flat0": {"ICL_CONV_SPLIT_FLAT": "0", "ICL_CONV_SPLIT_FLAT12": "0", "ICL_CONV_SPLIT_FLAT6": "0"},
    "flat24_0": {"ICL_CONV_SPLIT_FLAT": "0"},
    "flat12_0": {"ICL_CONV_SPLIT_FLAT12": "0"},
    "flat6_0": {"ICL_CONV_SPLIT_FLAT6": "0"},
    "min1": {"ICL_CONV_SPLIT_MIN": "1"},
}
BATCHES = (1, 2, 4)


def table(L, setenv, delenv):
    """{"setting|n|cin|cout|edge": [fwd_ws_bytes ks 3, ks 1, presplit_ws_bytes, stats_slots, wgrad_ws_bytes ks 3, ks 1, [live_ok ...]]}"""
    out = {}
    for name, env in SETTINGS.items():
        for k in SWITCHES:
            delenv(k)
        for k, v in env.items():
            setenv(k, v)
        for n in BATCHES:
            for cin, cout, e in SHAPES:
                out[f"{name}|{n}|{cin}|{cout}|{e}"] = [
                    L.icl_conv3d_fwd_ws_bytes(n, cin, cout, e, e, e, 3), L.icl_conv3d_fwd_ws_bytes(n, cin, cout, e, e, e, 1),
                    L.icl_conv3d_fwd_presplit_ws_bytes(n, cin, cout, e, e, e), L.icl_conv3d_fwd_stats_slots(n, cin, cout, e, e, e),
                    L.icl_conv3d_wgrad_ws_bytes(n, cin, cout, 3), L.icl_conv3d_wgrad_ws_bytes(n, cin, cout, 1),
                    [L.icl_conv3d_fwd_live_ok(n, k, cin, cout, e, e, e) for k in range(1, n + 1)]]
    for k in SWITCHES:
        delenv(k)
    return out


@pytest.fixture()
def emu_library():
    from build_emu import build_emu
    _lib._use_library_for_tests(build_emu(), host_pointers=True)
    yield _lib.lib()
    _lib._use_library_for_tests(None)


def test_queries_answer_as_before_the_planner(monkeypatch, emu_library):
    with open(GOLDEN) as f:
        want = json.load(f)
    got = table(emu_library, monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False))
    assert len(want) == len(SETTINGS) * len(BATCHES) * len(SHAPES) and sorted(got) == sorted(want)      # no row left out
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, (len(wrong), dict(list(wrong.items())[:6]))
    # the rows the change was specified with (batch 2, default switches): 64->64 @24^3, 192->64 @24^3, 16->16 @96^3
    assert got["default|2|64|64|24"][0:1] + got["default|2|64|64|24"][2:4] + got["default|2|64|64|24"][6:] == [21233664, 0, 72, [0, 1]]
    assert got["default|2|192|64|24"][0:1] + got["default|2|192|64|24"][2:4] + got["default|2|192|64|24"][6:] == [23445504, 21233664, 0, [0, 0]]
    assert got["default|2|16|16|96"][0:1] + got["default|2|16|16|96"][2:4] + got["default|2|16|16|96"][6:] == [46080, 0, 256, [1, 1]]
